"""Iterations/s of whole 40-iteration solves of FW_l0l1_log_and_linear_step on the l2 ball with LogisticRegression, on one
MI355X in one process, by three routes through an iteration:

  generic   fused=False                 the composition of existing calls: func_grad, the oracle, s - x, three inner
                                        products with a read-back each, one pass over A per trial
  fused     fused=True                  the direction step in one call and one read-back (accbpg_fw_direction)
  carried   fused=True, carry=True      and the margins carried along the segment: A d once, every trial O(m)

Shapes: (4096,32768) and (65536,2048), 1 GiB of A each (those of tools/logistic_rate.py).  The routes alternate, three
timed runs each after an untimed one; every figure is the median and the min-max.  The yardstick is `generic`: the
parent commit has no such solver to time.  `trials_per_iteration` is the mean number of line-search trials; the passes
over A predict 2 + trials against 2.  A route pays when its median lies outside the other's min-max spread
(`*_pays`).  It is a record, not a gate: the exit status is 0.

Usage:  python tools/l0l1_rate.py [--out profiles/l0l1_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

ITERS = 40
RUNS = 3
ROUTES = (("generic", dict(fused=False)), ("fused", dict(fused=True)), ("carried", dict(fused=True, carry=True)))


def stats(v):
    return {"median": round(float(np.median(v)), 2), "min": round(float(min(v)), 2), "max": round(float(max(v)), 2)}


def instance(m, n):
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    w = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    y = torch.where(A @ w > 0, 1.0, -1.0).to(torch.float64)
    L1 = float(torch.linalg.norm(A, dim=1).max())
    return A, y, L1


def solve(f, L1, n, kw):
    x0 = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = acc.FW_l0l1_log_and_linear_step(f, acc.SquaredL2Norm(), 1e-12, L1, x0, ITERS, acc.lmo_l2_ball(1.0), 2.0,
                                          verbose=False, **kw)
    torch.cuda.synchronize()
    return len(out[1]) / (time.perf_counter() - t), out


def shape_record(m, n):
    A, y, L1 = instance(m, n)
    f = acc.LogisticRegression(A, y)
    rates = {name: [] for name, _ in ROUTES}
    trials = {}
    for run in range(RUNS + 1):
        for name, kw in ROUTES:
            rate, out = solve(f, L1, n, kw)
            if run > 0:                                         # (the first run of each route is not timed)
                rates[name].append(rate)
            trials[name] = (len(out[3]) - 1) / len(out[1])
    rec = {"shape": [m, n], "iterations": ITERS, "runs": RUNS,
           "iterations_per_s": {k: stats(v) for k, v in rates.items()},
           "trials_per_iteration": {k: round(v, 3) for k, v in trials.items()}}
    g, fu, ca = (rec["iterations_per_s"][k] for k in ("generic", "fused", "carried"))
    rec["fused_pays"] = bool(fu["median"] > g["max"])
    rec["carried_pays"] = bool(ca["median"] > fu["max"] and ca["median"] > g["max"])
    rec["passes_predicted_generic_over_carried"] = round((2 + trials["generic"]) / 2, 3)
    rec["measured_carried_over_generic"] = round(ca["median"] / g["median"], 3)
    rec["measured_fused_over_generic"] = round(fu["median"] / g["median"], 3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0), "solver": "FW_l0l1_log_and_linear_step, lmo_l2_ball(1.0), ls_ratio 2",
           "shapes": [shape_record(4096, 32768), shape_record(65536, 2048)]}
    text = json.dumps(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(rec, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
