"""A/B of the k-loop of the 64x64 tile products (accbpg_debug_gemm_loop) in one process: after a warm-up, rounds of
gradient evaluations alternate between the variants, and the HIP-event time of the inverse merges (profile category
`trtri`) per evaluation is recorded for each.  Variant 1 is the loop with one k-step of look-ahead, 0 is production,
2..4 keep that many k-steps of global loads in flight.  Value and gradient must be the same bits under every variant."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2048x32768,512x8192,1024x8192")
    ap.add_argument("--variants", default="1,0", help="switch values, measured in this order in every round")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--evals", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    variants = [int(v) for v in args.variants.split(",")]
    res = []
    try:
        for shp in args.shapes.split(","):
            m, n = (int(v) for v in shp.split("x"))
            gen = torch.Generator(device="cuda").manual_seed(7)
            V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
            x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
            x /= x.sum()
            f = acc.DOptimalObj(V)
            f.overlap_values(False)
            ref = None
            for v in variants:                                          # warm-up, and the bits
                assert lib.accbpg_debug_gemm_loop(v) == 0
                fx, g = f.func_grad(x, 2)
                if ref is None:
                    ref = (fx, g.clone())
                assert fx == ref[0] and torch.equal(g, ref[1]), "variant %d changes the result at %s" % (v, shp)
            rec = {"shape": [m, n], "evals_per_round": args.evals, "bit_identical": True,
                   "trtri_ms": {str(v): [] for v in variants}}
            for rnd in range(args.rounds):
                for v in variants:
                    lib.accbpg_debug_gemm_loop(v)
                    f.profile(True)
                    for _ in range(args.evals):
                        f.func_grad(x, 2)
                    tot, cnt = f.profile_read()["trtri"]
                    f.profile(False)
                    rec["trtri_ms"][str(v)].append(tot / args.evals)
            for v in variants:
                t = rec["trtri_ms"][str(v)]
                rec["variant_%d" % v] = {"median_ms": float(np.median(t)), "min_ms": min(t), "max_ms": max(t)}
            print(json.dumps(rec), flush=True)
            res.append(rec)
            del f, V
            torch.cuda.empty_cache()
    finally:
        lib.accbpg_debug_gemm_loop(0)
    if args.out:
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
