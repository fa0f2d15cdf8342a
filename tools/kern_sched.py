"""A/B of the schedules of the direct-to-LDS Gram and gradient kernels in ONE process, interleaved rounds
(cdna_hip_programming.md 5.4 rule 24): variant 0 = reads and multiplies issued as a block at every fragment-group
boundary, 1 = dealt out between MFMA pairs (reads behind odd pairs, loads behind even pairs, barrier in the middle of the
last group; timing code 18, no longer in the table), 2 = dealt out with the reads early in the group and the barrier behind
the first fragment row, one load per M0 write through the builtin; 3 / 4 = variant 2 with the loads of the k-loop two
/ four to an M0 write (timing codes 28, 29), 5 = variant 3 with the stage of every k-step a compile-time constant (production,
timing code 30; 3 is that loop rolled over a runtime stage index, production before).  --batch K times the Gram codes on
instance 0 of a lock-step batch of K (the shape a batch instance runs at, e.g. --m 512 --n 8192); --gram-only leaves the
gradient kernel out.  The handle's switch, used for the bit-identity check and the gradient kernel's
timings: Gram 0 = production, 1 = builtin loads, 2 = four to an M0 write, 3 = block schedule; gradient kernel 0 =
production (rectangular and diagonal phase per row block, one pipeline per workgroup), 1 = builtin loads, 2 = dealt out,
3 = the production schedule before the two phases (runtime triangular skip, pipeline restarted per row block).
Checks first that value and gradient are bit-identical under every variant."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=2048)
    ap.add_argument("--n", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=0, help="time instance 0 of a lock-step batch of this many instances")
    ap.add_argument("--gram-only", action="store_true")
    args = ap.parse_args()
    import torch
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import _ptr
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(3)
    V = torch.randn(args.m, args.n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(args.n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    if args.batch:
        from accbpg_and_fw_amd.batched import DOptimalBatch
        Vs = [V] + [torch.randn(args.m, args.n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(args.batch - 1)]
        batch = DOptimalBatch(Vs)
        assert batch.fused
        f = batch.instance(0)
    else:
        f = acc.DOptimalObj(V)
        f.overlap_values(False)
    base = f.func_grad(x, 2)
    same = {}
    for v in (1, 2, 3, "rolled", 0):
        lib.accbpg_debug_chol_variant(f._h, 1024 if v == "rolled" else v << 30)   # bit 10: schedule 0 on the rolled loop
        r = f.func_grad(x, 2)
        same[v] = bool(r[0] == base[0] and torch.equal(r[1], base[1]))
    print("bit-identical:", same, flush=True)
    out = {"shape": [args.m, args.n], "batch": args.batch, "bit_identical": same, "gram_ms": {}, "grad_ms": {}}
    ms = C.c_double(0.0)
    codes = {3: 28, 5: 30} if args.gram_only else {0: 10, 2: 19, 3: 28, 4: 29, 5: 30}
    for rnd in range(args.rounds):
        for v, code in codes.items():
            _lib.check(lib.accbpg_debug_gram_variant(f._h, _ptr(x), code, args.iters, C.byref(ms)), "gram variant")
            out["gram_ms"].setdefault(v, []).append(ms.value)
        for v in (() if args.gram_only else (0, 1, 2, 3)):
            lib.accbpg_debug_chol_variant(f._h, v << 30)             # gradient kernel: 0 production, 1 builtin loads, 2 dealt out, 3 before the phases
            f.profile(True)
            for _ in range(args.iters):
                f.func_grad(x, 1)
            tot, cnt = f.profile_read()["grad"]
            f.profile(False)
            out["grad_ms"].setdefault(v, []).append(tot / cnt)
        print(rnd, {v: round(out["gram_ms"][v][-1], 4) for v in codes}, {v: round(t[-1], 4) for v, t in out["grad_ms"].items()},
              flush=True)
    lib.accbpg_debug_chol_variant(f._h, 0)
    for key in ("gram_ms", "grad_ms"):
        out[key + "_median"] = {v: float(np.median(t)) for v, t in out[key].items()}
        out[key + "_min"] = {v: float(np.min(t)) for v, t in out[key].items()}
        out[key + "_max"] = {v: float(np.max(t)) for v, t in out[key].items()}
    txt = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt)
    print(txt)


if __name__ == "__main__":
    main()
