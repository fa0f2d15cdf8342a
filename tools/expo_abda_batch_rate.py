"""The lock-step batches of ABPG_expo and ABDA against the route that existed before them, on the same instances in one
process:

  batch   ABPG_expo_batch / ABDA_batch on a DOptimalBatch (one launch per kernel family and pass for all running
          instances; ABDA's sum, quotient and prox in one launch)
  loop    ABPG_expo / ABDA on batch.instance(i) for i = 0 .. K-1, one after the other, on the handles of that batch --
          the code a user of these two solvers had before the batches
  alone   (with --alone) the same loop on stand-alone DOptimalObj handles over the same matrices: planned for one
          instance on the whole chip, so not bit-identical to the batch (another order of summation in the Gram
          product); the largest relative difference of F between it and the batch is recorded

K = 64 instances of D_opt_design(512, 8192) and K = 4 of (2048, 32768): the matrices of D_opt_design(m, n,
randseed=11+i), L = 1, gamma0 = 3 (ABPG_expo) / gamma = 2 (ABDA), the solvers' defaults otherwise, from the uniform
start.  Every run is a whole solve of all K instances timed by the wall clock (no warm-up iterations; the batch and its
handles are built before the clock starts, and one untimed 2-iteration solve per route has made the lazy allocations);
the runs alternate between the routes and are reported as median / min / max of instance-iterations per second.  Both
routes run on the same handles, so their results are compared bit for bit.

Usage:  python tools/expo_abda_batch_rate.py [--out profiles/expo_abda_batch_rate.json] [--iters 40] [--runs 3]
                                             [--cases 512x8192x64,2048x32768x4] [--alone]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--cases", default="512x8192x64,2048x32768x4")
ap.add_argument("--alone", action="store_true")
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


def solver_record(batch, h, x0, iters, runs, batch_fn, loop_fn, alone):
    K = batch.K
    route = {"batch": lambda it: batch_fn(batch, h, 1.0, x0, maxitrs=it),
             "loop": lambda it: [loop_fn(batch.instance(i), h, 1.0, x0, maxitrs=it, verbose=False) for i in range(K)]}
    if alone:
        route["alone"] = lambda it: [loop_fn(f, h, 1.0, x0, maxitrs=it, verbose=False) for f in alone]
    for fn in route.values():
        fn(2)
    rates = {name: [] for name in route}
    identical, rel = True, 0.0
    for _ in range(runs):
        got = {}
        for name, fn in route.items():
            dt, got[name] = timed(lambda: fn(iters))
            rates[name].append(sum(len(r[1]) for r in got[name]) / dt)
        for a, b in zip(got["batch"], got["loop"]):
            identical = identical and all(np.array_equal(u, v) for u, v in zip(a[:-1], b[:-1]))
        for a, b in zip(got["batch"], got.get("alone", [])):
            if len(a[1]) == len(b[1]):                           # (else: it stopped elsewhere; the rate still counts its own)
                rel = max(rel, float(np.max(np.abs(a[1] - b[1]) / np.abs(b[1]))))
    rec = {name: spread(r) for name, r in rates.items()}
    rec["bit_identical"] = bool(identical)
    rec["batch_over_loop_median"] = round(rec["batch"]["median"] / rec["loop"]["median"], 3)
    if alone:
        rec["batch_over_alone_median"] = round(rec["batch"]["median"] / rec["alone"]["median"], 3)
        rec["F_max_rel_diff_batch_alone"] = rel
    return rec


def case(m, n, K, iters, runs):
    Vs = []
    for i in range(K):
        np.random.seed(11 + i)                                   # the matrix of D_opt_design(m, n, randseed=11+i)
        Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    h = acc.BurgEntropySimplex()
    alone = [acc.DOptimalObj(V) for V in Vs] if ARGS.alone else None
    rec = {"shape": [m, n], "K": K, "iters": iters}
    rec["ABPG_expo"] = solver_record(batch, h, x0, iters, runs,
                                     lambda *a, **k: acc.ABPG_expo_batch(*a, gamma0=3, **k),
                                     lambda *a, **k: acc.ABPG_expo(*a, gamma0=3, **k), alone)
    print("# %dx%d K=%d ABPG_expo %s" % (m, n, K, json.dumps(rec["ABPG_expo"])), flush=True)
    rec["ABDA"] = solver_record(batch, h, x0, iters, runs,
                                lambda *a, **k: acc.ABDA_batch(*a, gamma=2, **k),
                                lambda *a, **k: acc.ABDA(*a, gamma=2, **k), alone)
    print("# %dx%d K=%d ABDA %s" % (m, n, K, json.dumps(rec["ABDA"])), flush=True)
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
        "method": "wall clock around the whole solve of all K instances (no warm-up iterations; one untimed 2-iteration "
                  "solve per route first), D_opt_design(m, n, randseed=11+i), L = 1, gamma0 = 3 (ABPG_expo) / gamma = 2 "
                  "(ABDA), solver defaults, uniform x0; batch = ABPG_expo_batch / ABDA_batch, loop = ABPG_expo / ABDA on "
                  "batch.instance(i) one after the other, alone (if present) = the same loop on stand-alone DOptimalObj "
                  "handles; runs alternate between the routes; median / min / max over the runs",
    }
    s = json.dumps(rec)
    print(s)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
