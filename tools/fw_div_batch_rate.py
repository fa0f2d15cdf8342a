"""The lock-step Bregman-step Frank-Wolfe batch against the one route that existed before it, on the same instances in
one process:

  batch   D_opt_FW_div_step_batch on a DOptimalBatch (one launch per step kernel and one synchronisation per iteration
          for all instances)
  loop    D_opt_FW_div_step(batch.instance(i), ...) for i = 0 .. K-1, one after the other, on the handles of that batch

K = 8 and K = 64 instances of D_opt_design(512, 8192), K = 4 of (2048, 32768): the matrices of
D_opt_design(m, n, randseed=11+i), L = 1, gamma = 2, line search on, the default refresh, 200 iterations from the uniform
start.  Every run is a whole solve of all K instances timed by the wall clock (initialisation included, no warm-up
iterations; the batch and its handles are built before the clock starts); three runs per route, alternating, reported
as median / min / max.  Both routes run on the same handles, so F is compared bit for bit as well as by its largest
relative difference.

Usage:  python tools/fw_div_batch_rate.py [--out profiles/fw_div_batch_rate.json] [--iters 200] [--runs 3]
                                          [--cases 512x8192x8,512x8192x64,2048x32768x4]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--cases", default="512x8192x8,512x8192x64,2048x32768x4")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(rates):
    return {"median": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}


def case(m, n, K, iters, runs):
    Vs = []
    for i in range(K):
        np.random.seed(11 + i)                                   # the matrix of D_opt_design(m, n, randseed=11+i)
        Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    rates = {"batch": [], "loop": []}
    rel, identical = 0.0, True
    for _ in range(runs):
        dt, res = timed(lambda: acc.D_opt_FW_div_step_batch(batch, 1.0, x0, iters, 2.0))
        rates["batch"].append(sum(len(r[1]) for r in res) / dt)
        dt, ref = timed(lambda: [acc.D_opt_FW_div_step(batch.instance(i), 1.0, x0, iters, 2.0, verbose=False)
                                 for i in range(K)])
        rates["loop"].append(sum(len(r[1]) for r in ref) / dt)
        for a, b in zip(res, ref):
            assert len(a[1]) == len(b[1]), "the two routes ran different numbers of iterations"
            rel = max(rel, float(np.max(np.abs(a[1] - b[1]) / np.abs(b[1]))))
            identical = identical and np.array_equal(a[1], b[1]) and np.array_equal(a[0], b[0])
    rec = {"shape": [m, n], "K": K, "iters": iters, "batch": spread(rates["batch"]), "loop": spread(rates["loop"]),
           "F_max_rel_diff_between_routes": rel, "x_and_F_bit_identical": bool(identical)}
    rec["batch_over_loop_median"] = round(rec["batch"]["median"] / rec["loop"]["median"], 3)
    rec["batch_median_minus_loop_median"] = round(rec["batch"]["median"] - rec["loop"]["median"], 1)
    rec["loop_min_max_spread"] = round(rec["loop"]["max"] - rec["loop"]["min"], 1)
    return rec


def main():
    cases = []
    for spec in ARGS.cases.split(","):
        m, n, K = (int(v) for v in spec.split("x"))
        cases.append(case(m, n, K, ARGS.iters, ARGS.runs))
        torch.cuda.empty_cache()
    rec = {
        "device": torch.cuda.get_device_name(0), "unit": "instance-iterations per second", "runs": ARGS.runs,
        "cases": cases,
        "method": "wall clock around the whole solve of all K instances (initialisation included, no warm-up), "
                  "D_opt_design(m, n, randseed=11+i), L = 1, gamma = 2, line search on, default refresh, uniform x0; "
                  "batch = D_opt_FW_div_step_batch, loop = D_opt_FW_div_step on batch.instance(i) one after the other; "
                  "runs alternate between the routes; median / min / max over the runs",
    }
    s = json.dumps(rec)
    print(s)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
