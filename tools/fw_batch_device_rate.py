"""Aggregate iterations per second of the Frank-Wolfe D-optimal solvers on K instances of one shape, by three routes
in one process, on the same matrices, for the same fixed number of iterations (eps = 0: the stop test never holds):

  (a) lockstep       D_opt_FW_batch / D_opt_FW_away_batch: one launch per step kernel for all instances, the host takes
                     every decision (one blocking round trip per iteration)
  (b) device_single  K consecutive D_opt_FW_device / D_opt_FW_away_device runs on the batch's instances: the decisions
                     of 64 (R = 16 for the away variant) iterations on the device, one instance at a time
  (c) batch_device   D_opt_FW_batch_device / D_opt_FW_away_batch_device at sync_every = 16 and 64 (away: R = 16, which
                     cuts the chunks at 16): one launch per step kernel for all instances AND the decisions on the device

Each route is timed --reps times after a warm-up run; the record holds the median and the min-max spread of
K * iterations / wall time, and the ratios of the medians of (c) to (a) and to (b).  Every run of (c) -- the warm-up and
the timed ones -- is asserted bit-identical (x, F, SP, SN) to (a).  At K = 4 x (2048,32768), where the pass over V
dominates, the acceptance condition is recorded: the median of (c) is not below the median of (a) by more than the
min-max spread of (a).

Usage:  python tools/fw_batch_device_rate.py [--out profiles/fw_batch_device_rate.json] [--reps 5] [--cases ...]
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

# m x n x K x iterations
CASES = "30x1000x8x2000,30x1000x64x2000,512x8192x8x1000,512x8192x64x1000,2048x32768x4x500"


def identical(res, ref):
    return all(np.array_equal(p, q, equal_nan=True) for r, s in zip(res, ref) for p, q in zip(r[:4], s[:4]))


def timed(fn, K, iters, reps, ref=None):
    """aggregate it/s of ``fn()`` (a whole solve of K instances, ``iters`` iterations each): median, min, max over
    ``reps`` runs after one; every run compared with ``ref`` when given"""
    out = fn()
    assert len(out) == K and all(len(r[1]) == iters for r in out)
    assert ref is None or identical(out, ref), "differs from the lock-step run"
    rates = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        rates.append(K * iters / (time.perf_counter() - t))
        assert ref is None or identical(res, ref), "differs from the lock-step run"
    return {"median": round(float(np.median(rates)), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}, out


def case(m, n, K, iters, reps):
    Vs = []
    for i in range(K):
        np.random.seed(11 + i)                                   # the matrix of D_opt_design(m, n, randseed=11+i)
        Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    row = {"shape": [m, n], "K": K, "iterations": iters}
    for name, lock, single, dev, kw in (
            ("fw", acc.D_opt_FW_batch, acc.D_opt_FW_device, acc.D_opt_FW_batch_device, {}),
            ("away_R16", acc.D_opt_FW_away_batch, acc.D_opt_FW_away_device, acc.D_opt_FW_away_batch_device,
             {"logdet_refresh": 16})):
        a, ref = timed(lambda: lock(batch, x0, 0.0, iters, **kw), K, iters, reps)
        b, _ = timed(lambda: [single(batch.instance(i), x0, 0.0, iters, verbose=False, **kw) for i in range(K)],
                     K, iters, reps, ref)
        r = {"lockstep_it_per_s": a, "device_single_it_per_s": b}
        for S in (16, 64):
            c, _ = timed(lambda: dev(batch, x0, 0.0, iters, sync_every=S, **kw), K, iters, reps, ref)
            c["ratio_to_lockstep"] = round(c["median"] / a["median"], 3)
            c["ratio_to_device_single"] = round(c["median"] / b["median"], 3)
            r["batch_device_S%d_it_per_s" % S] = c
        if (m, n) == (2048, 32768):
            floor = a["median"] - (a["max"] - a["min"])
            r["acceptance"] = {"floor_it_per_s": round(floor, 1),
                               "met": {k: bool(v["median"] >= floor) for k, v in r.items() if k.startswith("batch_device_")}}
        row[name] = r
    del batch
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fw_batch_device_rate.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for spec in a.cases.split(","):
        m, n, K, iters = (int(v) for v in spec.split("x"))
        rows.append(case(m, n, K, iters, a.reps))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "unit": "instance-iterations per second",
           "method": "wall clock of whole solves of all K instances (initialisation included, eps=0, uniform x0, "
                     "D_opt_design(m, n, randseed=11+i)), %d runs after a warm-up run; x, F, SP, SN of every "
                     "device_single and batch_device run asserted bit-identical to the lock-step run" % a.reps,
           "cases": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
