"""SVM_fun.func_grad against PoissonRegression.func_grad at the same shapes, on one MI355X in one process: flags 0 and
2 of both (the two share both passes over A and differ in the per-row epilogue, the value's second sum and the
elementwise gradient combine), vec_axpby at length n, and the iterations/s of the two ex_SVM drivers' solver calls on
the device against the NumPy restatement on the same box.

Shapes: (700,2000), the reference's own generated instance, and (8192,65536).  Every figure is the median and the
min-max of 5 runs after a warm-up, the objectives interleaved run by run.  Acceptance, at (8192,65536) only: SVM's
flag-2 median must not exceed Poisson's median by more than Poisson's own min-max spread plus the measured vec_axpby
time (the passes move the same bytes and the hinge epilogue has no log; the gradient combine is one more length-n pass).

Usage:  python tools/svm_rate.py [--out profiles/svm_rate.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd.functions import vec_axpby  # noqa: E402

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


def shape_record(m, n, reps):
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=gen)
    A /= A.sum(dim=0)
    xt = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    b = A @ xt + 1e-3
    y = torch.where(A @ (xt - xt.mean()) > 0, 1.0, -1.0).to(torch.float64)
    x = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
    fs, fp = acc.SVM_fun(0.1, A, y), acc.PoissonRegression(A, b)
    t = timed([lambda: fs.func_grad(x, 0), lambda: fs.func_grad(x, 2), lambda: fp.func_grad(x, 0),
               lambda: fp.func_grad(x, 2), lambda: vec_axpby(0.5, x, 0.5, xt)], reps)
    rec = {"shape": [m, n], "reps_per_run": reps,
           "svm_flag0_ms": stats(t[0]), "svm_flag2_ms": stats(t[1]), "poisson_flag0_ms": stats(t[2]),
           "poisson_flag2_ms": stats(t[3]), "vec_axpby_ms": stats(t[4])}
    by = 2 * 8 * m * n
    rec["share_of_hbm_peak_flag2"] = {"svm": round(by / (np.median(t[1]) * 1e-3) / HBM_PEAK, 4),
                                      "poisson": round(by / (np.median(t[3]) * 1e-3) / HBM_PEAK, 4)}
    return rec


def driver_rates(iters):
    """iterations/s of the ex_SVM solver calls (poly_h, `iters` iterations) on the generated (700,2000) instance: the
    device package against the NumPy restatement, both called with NumPy vectors as the drivers call them"""
    import svm_numpy as SN
    np.random.seed(3)
    X, Y = acc.generate_dataset_for_svm(700, 2000)
    out = {}
    for name in SN.driver_table(SN.SOLVERS, SN.lmo_l2_ball):
        lamda = 0.001 if name in ("aibm", "fgm") else 0.01
        np.random.seed(3)
        radius, _, _, L, x0 = SN.ball_numbers(X, Y, lamda)
        rates = {}
        for tag, mod, lmo, fcls, hcls in (("device", acc, acc.lmo_l2_ball, acc.SVM_fun, acc.PolyDiv),
                                          ("numpy", SN.SOLVERS, SN.lmo_l2_ball, SN.SVM_fun, SN.PolyDiv)):
            f, ph = fcls(lamda, X, Y), hcls(X, lamda=lamda, radius=radius)
            call = SN.driver_table(mod, lmo, iters)[name]
            v = []
            for r in range(RUNS + 1):
                np.random.seed(77)
                with contextlib.redirect_stdout(io.StringIO()):
                    if tag == "device":
                        torch.cuda.synchronize()
                    t = time.perf_counter()
                    res = call(f, ph, L, np.copy(x0), radius)
                    if tag == "device":
                        torch.cuda.synchronize()
                    dt = time.perf_counter() - t
                if r:
                    v.append(len(res[1]) / dt)
            rates[tag] = stats(v)
            rates[tag]["iterations"] = len(res[1])
        rates["ratio_device_over_numpy"] = round(rates["device"]["median"] / rates["numpy"]["median"], 3)
        out[name] = rates
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    small, big = shape_record(700, 2000, 200), shape_record(8192, 65536, 10)
    slack = (big["poisson_flag2_ms"]["max"] - big["poisson_flag2_ms"]["min"]) + big["vec_axpby_ms"]["median"]
    excess = big["svm_flag2_ms"]["median"] - big["poisson_flag2_ms"]["median"]
    rec = {"device": torch.cuda.get_device_name(0), "shapes": [small, big],
           "acceptance_8192x65536": {"svm_minus_poisson_ms": round(excess, 5), "allowed_ms": round(slack, 5),
                                     "holds": bool(excess <= slack)},
           "ex_SVM_it_per_s_700x2000": driver_rates(a.iters),
           "method": "median and min-max of %d runs after a warm-up, one process, objectives interleaved run by run; "
                     "wall clock around calls that each wait for their value (flag 0, 2) or a closing synchronise"
                     % RUNS}
    s = json.dumps(rec, indent=1)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")
    return 0 if rec["acceptance_8192x65536"]["holds"] else 1


if __name__ == "__main__":
    sys.exit(main())
