"""LogisticRegression.func_grad against SVM_fun.func_grad on the same matrices, on one MI355X in one process: flags 0
and 2 of both (the two share both passes over A and differ in the per-row epilogue of pass 1, which runs once per
row), and the iterations/s of ABPG_gain as accbpg/ex_LR_L2L1Linf.py calls it.  svm_kernels.hip is the parent commit's
file unchanged, so its times here are the parent's.

Shapes: (4096,32768) and (65536,2048), 1 GiB of A each; ABPG_gain at the example's (100,200) and at (4096,32768).
Every figure is the median and the min-max of 5 runs after a warm-up, the objectives interleaved run by run.  The
expectation is SVM's time; `gap_beyond_svm_spread` says whether the logistic median leaves SVM's own min-max spread.
It is a record, not a gate: the exit status is 0.

Usage:  python tools/logistic_rate.py [--out profiles/logistic_rate.json]
Prints one JSON object (and writes it to --out)."""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

HBM_PEAK = 8.0e12       # bytes/s, the figure DESIGN.md holds the other passes to
RUNS = 5


def stats(v):
    return {"median": round(float(np.median(v)), 5), "min": round(float(min(v)), 5), "max": round(float(max(v)), 5)}


def timed(calls, reps):
    """ms per call of each callable: RUNS runs of `reps` calls after a warm-up, interleaved run by run"""
    out = [[] for _ in calls]
    for c in calls:
        for _ in range(3):
            c()
    for _ in range(RUNS):
        for k, c in enumerate(calls):
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                c()
            torch.cuda.synchronize()
            out[k].append((time.perf_counter() - t) / reps * 1e3)
    return out


def instance(m, n):
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    w = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen)
    y = torch.where(A @ w > 0, 1.0, -1.0).to(torch.float64)
    x = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) / n ** 0.5
    return A, y, x


def shape_record(m, n, reps):
    A, y, x = instance(m, n)
    fl, fs = acc.LogisticRegression(A, y), acc.SVM_fun(0.0, A, y)
    t = timed([lambda: fl.func_grad(x, 0), lambda: fl.func_grad(x, 2), lambda: fs.func_grad(x, 0),
               lambda: fs.func_grad(x, 2)], reps)
    rec = {"shape": [m, n], "reps_per_run": reps, "logistic_flag0_ms": stats(t[0]), "logistic_flag2_ms": stats(t[1]),
           "svm_flag0_ms": stats(t[2]), "svm_flag2_ms": stats(t[3])}
    by = 2 * 8 * m * n
    rec["share_of_hbm_peak_flag2"] = {"logistic": round(by / (np.median(t[1]) * 1e-3) / HBM_PEAK, 4),
                                      "svm": round(by / (np.median(t[3]) * 1e-3) / HBM_PEAK, 4)}
    rec["share_of_hbm_peak_flag0"] = {"logistic": round(by / 2 / (np.median(t[0]) * 1e-3) / HBM_PEAK, 4),
                                      "svm": round(by / 2 / (np.median(t[2]) * 1e-3) / HBM_PEAK, 4)}
    for flag in ("flag0", "flag2"):
        lg, sv = rec["logistic_%s_ms" % flag], rec["svm_%s_ms" % flag]
        rec["gap_beyond_svm_spread_" + flag] = bool(lg["median"] > sv["max"] or lg["median"] < sv["min"])
    return rec


def gain_rate(m, n, iters):
    """iterations/s of ABPG_gain(f, L2L1Linf(1/m, 1), 0.25, zeros, gamma=2, restart=False), NumPy x0 as the example's"""
    if (m, n) == (100, 200):
        f, h, L, x0 = acc.Logistic_regr_L2L1Linf(m, n, randseed=1)
    else:
        A, y, _ = instance(m, n)
        f, h, L, x0 = acc.LogisticRegression(A, y), acc.L2L1Linf(lamda=1.0 / m, B=1), 0.25, np.zeros(n)
    v = []
    for r in range(RUNS + 1):
        with contextlib.redirect_stdout(io.StringIO()):
            torch.cuda.synchronize()
            t = time.perf_counter()
            res = acc.ABPG_gain(f, h, L, np.copy(x0), gamma=2, maxitrs=iters, restart=False, verbskip=10)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
        if r:
            v.append(len(res[1]) / dt)
    out = stats(v)
    out.update({"shape": [m, n], "iterations": len(res[1])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0),
           "shapes": [shape_record(4096, 32768, 10), shape_record(65536, 2048, 10)],
           "ABPG_gain_it_per_s": [gain_rate(100, 200, a.iters), gain_rate(4096, 32768, a.iters)],
           "method": "median and min-max of %d runs after a warm-up, one process, objectives interleaved run by run; "
                     "wall clock around calls that each wait for their value; SVM_fun is the parent commit's code"
                     % RUNS}
    s = json.dumps(rec, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
