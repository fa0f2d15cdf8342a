"""Lock-step Frank-Wolfe batches against the routes that existed before them, on the same instances in one process:

  batch       D_opt_FW_batch / D_opt_FW_away_batch on a DOptimalBatch (one launch per step kernel, one synchronisation
              per step for all instances)
  threads     solve_batch(..., D_opt_FW / D_opt_FW_away) with 8 host threads, one stream per instance
  sequential  a plain loop over the instances

K = 8 and K = 64 instances of D_opt_design(512, 8192), K = 4 of (2048, 32768); every route runs the same number of
iterations (eps = -1: no instance stops) from the uniform start, timed by the wall clock around the whole solve
(initialisation included, no warm-up iterations; objectives and handles are built before the clock starts).

`--root DIR` imports the package from another checkout (with its library built) -- that is how the baseline routes of
the commit BEFORE the batch are measured on the same box: run `--routes threads,sequential --root PARENT --out B.json`
there, then the batch here with `--baseline B.json`, which is embedded in the record.

Usage:  python tools/fw_batch_rate.py [--out FILE.json] [--routes batch,threads,sequential] [--root DIR]
                                      [--baseline FILE.json] [--iters 300] [--iters-large 200]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--routes", default="batch,threads,sequential")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--baseline", default=None)
ap.add_argument("--iters", type=int, default=300)
ap.add_argument("--iters-large", type=int, default=200)
ap.add_argument("--cases", default="512x8192x8,512x8192x64,2048x32768x4")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd.batched import solve_batch  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def case(m, n, K, iters, routes):
    Vs = []
    for i in range(K):
        np.random.seed(11 + i)                                   # the matrix of D_opt_design(m, n, randseed=11+i)
        Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
    x0 = np.ones(n) / n
    rec = {"shape": [m, n], "K": K, "iters": iters}
    finals = {}
    for name in ("FW", "FW_away"):
        single = acc.D_opt_FW if name == "FW" else acc.D_opt_FW_away
        r = {}
        if "batch" in routes:
            batch = acc.DOptimalBatch(Vs)
            bsolver = acc.D_opt_FW_batch if name == "FW" else acc.D_opt_FW_away_batch
            dt, res = timed(lambda: bsolver(batch, x0, -1.0, iters))
            assert all(len(t[1]) == iters for t in res)
            r["batch"] = K * iters / dt
            finals["batch"] = [float(t[1][-1]) for t in res]
            del batch
        if "threads" in routes or "sequential" in routes:
            objs = [acc.DOptimalObj(V) for V in Vs]
            probs = [(f, None, None, x0) for f in objs]
            run = lambda f, h, L, x: single(f, x, -1.0, iters, verbose=False)   # noqa: E731
            if "threads" in routes:
                dt, res = timed(lambda: solve_batch(probs, run, threads=8))
                r["threads8"] = K * iters / dt
                finals["threads8"] = [float(t[1][-1]) for t in res]
            if "sequential" in routes:
                dt, res = timed(lambda: [run(*p) for p in probs])
                r["sequential"] = K * iters / dt
                finals["sequential"] = [float(t[1][-1]) for t in res]
            del objs, probs
        # threads and sequential run on the same kind of handle: bit for bit.  The batch's instances are planned for
        # sharing the chip (256 x 128 Gram tiles also at m = 512, a capped stream-K grid), so their Gram matrices of x0
        # are summed in another order than a DOptimalObj's: against those F[-1] is held to the bar the trajectory
        # tests use between two summation orders (rtol 1e-9), and the distance is recorded.
        single = [finals[k] for k in ("threads8", "sequential") if k in finals]
        assert all(v == single[0] for v in single), "threads and sequential disagree on F[-1]"
        rec[name] = {k: round(v, 1) for k, v in r.items()}
        if "batch" in finals and single:
            rel = np.abs(np.array(finals["batch"]) - np.array(single[0])) / np.abs(np.array(single[0]))
            assert np.all(rel <= 1e-9), "the batch and the single handles disagree on F[-1] (max rel %.3e)" % rel.max()
            rec[name]["batch_F_last_max_rel_diff_to_single_handles"] = float(rel.max())
        finals.clear()
    return rec


def main():
    routes = ARGS.routes.split(",")
    cases = []
    for spec in ARGS.cases.split(","):
        m, n, K = (int(v) for v in spec.split("x"))
        cases.append(case(m, n, K, ARGS.iters if m < 2048 else ARGS.iters_large, routes))
        torch.cuda.empty_cache()
    rec = {
        "device": torch.cuda.get_device_name(0), "routes": routes, "unit": "instance-iterations per second",
        "cases": cases,
        "method": "wall clock around the whole solve of all K instances (initialisation included, no warm-up), eps = -1, "
                  "uniform x0, D_opt_design(m, n, randseed=11+i); D_opt_FW_away with its default logdet_refresh; every "
                  "route's F[-1] compared (threads8 and sequential bit for bit; the batch, whose instances use the batch's Gram "
                  "plan, within rtol 1e-9 of them)",
    }
    if ARGS.baseline:
        with open(ARGS.baseline) as fh:
            rec["baseline_before_the_batch"] = json.loads(fh.read())
    s = json.dumps(rec)
    print(s)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
