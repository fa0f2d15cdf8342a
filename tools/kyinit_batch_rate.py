"""Wall seconds of the Kumar-Yildirim starts of a DOptimalBatch computed one instance at a time (route 1: the loop
`for i: D_opt_KYinit_device(batch.instance(i))`) against all K in lock-step (route 2: D_opt_KYinit_batch(batch)), in one
process on one device, on the same batch and the same seed of the legacy generator, and beside them the wall time of
1000 D_opt_FW_away_batch_device iterations from that start -- what the starts are the prelude to.  Per (shape, K): each
route is timed --reps times after a warm-up run; the two routes must return equal arrays.

Usage:  python tools/kyinit_batch_rate.py [--out profiles/kyinit_batch_rate.json] [--reps 3]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import platform
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

CASES = [(512, 8192, 8), (512, 8192, 64), (2048, 32768, 4)]
SEED = 12
FW_ITERS = 1000


def wall(fn):
    np.random.seed(SEED)
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(ts):
    return {"median": round(float(np.median(ts)), 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "runs": len(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kyinit_batch_rate.json"))
    a = ap.parse_args()
    assert a.reps >= 3, "at least 3 runs per route"
    torch.cuda.set_device(0)
    rows = []
    for m, n, K in CASES:
        Vs = []
        for i in range(K):                                      # D_opt_design(m, n, randseed=10 + i), the matrix alone
            np.random.seed(10 + i)
            Vs.append(np.random.randn(m, n))
        batch = acc.DOptimalBatch(Vs)
        del Vs
        loop_fn = lambda: np.stack([acc.D_opt_KYinit_device(batch.instance(i)) for i in range(K)])     # noqa: E731
        batch_fn = lambda: acc.D_opt_KYinit_batch(batch)                                                # noqa: E731
        wall(loop_fn)                                           # warm-up
        loop = [wall(loop_fn) for _ in range(a.reps)]
        wall(batch_fn)
        lock = [wall(batch_fn) for _ in range(a.reps)]
        X0 = lock[0][1]
        for _, X in loop + lock:
            assert np.array_equal(X, X0), "the two routes (or two runs of one) returned different starts"
        t_loop, t_lock = [t for t, _ in loop], [t for t, _ in lock]
        print(json.dumps({"shape": [m, n], "K": K, "loop_s": t_loop, "batch_s": t_lock}), file=sys.stderr, flush=True)
        run_fw = lambda: acc.D_opt_FW_away_batch_device(batch, X0, 0.0, FW_ITERS)                      # noqa: E731
        out = wall(run_fw)[1]
        fw = [wall(run_fw)[0] for _ in range(a.reps)]
        row = {"shape": [m, n], "K": K, "loop_s": spread(t_loop), "batch_s": spread(t_lock),
               "loop_over_batch": round(float(np.median(t_loop) / np.median(t_lock)), 2),
               "batch_faster_than_loop": bool(np.median(t_lock) < np.median(t_loop)),
               "fw_away_batch_device_%d_iterations_s" % FW_ITERS: spread(fw),
               "fw_iterations_run_min": int(min(len(r[1]) for r in out)),
               "routes_array_equal": True, "support": [int(np.count_nonzero(x)) for x in X0]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del batch
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "method": "wall clock around whole calls ending in a device synchronise, np.random.seed(%d) before each; "
                     "instance i is np.random.seed(10 + i); randn(m, n); each route %d runs after a warm-up run; "
                     "route 1 (loop_s): D_opt_KYinit_device(batch.instance(i)) for every i; route 2 (batch_s): "
                     "D_opt_KYinit_batch(batch)" % (SEED, a.reps),
           "cases": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
