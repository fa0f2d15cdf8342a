"""A/B of the gradient kernel's k-step in ONE process, interleaved rounds: production (dealt out) against the same
two-phase loop on the block schedule (the loop before the step was dealt out), against the dealt-out placement production
does not use and against dealing out the rectangular steps only, through accbpg_debug_grad_variant (codes 0, 4, 5, 6).
Checks first that they all write the same bits.  Records every round, the median and the min-max per shape."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAMES = {0: "production (dealt out)", 4: "block schedule (before)", 5: "dealt out, other placement",
         6: "only the rectangular k-step dealt out"}


def one_shape(m, n, rounds, iters):
    import torch
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import _ptr
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(3)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    # below m = 768 a handle of its own takes the 64 x 64 tile; the 256 x 128 tile runs there for the instances of a
    # lock-step batch (config 4: (512,8192)), so the handle measured is an instance of a batch of two
    batch = None
    if m < 768:
        from accbpg_and_fw_amd.batched import DOptimalBatch
        batch = DOptimalBatch([V, V.clone()])
        assert batch.fused
        f = batch.instance(0)
    else:
        f = acc.DOptimalObj(V)
    base = f.func_grad(x, 2)                                     # leaves the inverse factor the launches read
    ms = C.c_double(0.0)
    same = {}
    for c in NAMES:
        g = torch.zeros(n, dtype=torch.float64, device="cuda")
        _lib.check(lib.accbpg_debug_grad_variant(f._h, _ptr(g), c, 1, C.byref(ms)), "variant %d" % c)
        torch.cuda.synchronize()
        same[NAMES[c]] = bool(torch.equal(g, base[1]))
    print("bit-identical to func_grad at (%d,%d):" % (m, n), same, flush=True)
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    t = {c: [] for c in NAMES}
    for rnd in range(rounds):
        for c in NAMES:
            _lib.check(lib.accbpg_debug_grad_variant(f._h, _ptr(g), c, iters, C.byref(ms)), "variant %d" % c)
            t[c].append(ms.value)
        print(rnd, {c: round(v[-1], 4) for c, v in t.items()}, flush=True)
    return {"shape": [m, n], "handle": "instance of a lock-step batch" if batch is not None else "single", "bit_identical": same, "rounds_ms": {NAMES[c]: v for c, v in t.items()},
            "median_ms": {NAMES[c]: float(np.median(v)) for c, v in t.items()},
            "min_max_ms": {NAMES[c]: [float(np.min(v)), float(np.max(v))] for c, v in t.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x32768,512x8192,1024x8192")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"rounds": args.rounds, "launches_per_round": args.iters, "shapes": []}
    for s in args.shapes.split(","):
        m, n = (int(v) for v in s.split("x"))
        res["shapes"].append(one_shape(m, n, args.rounds, args.iters))
    txt = json.dumps(res, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
