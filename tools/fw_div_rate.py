"""Iterations per second of Frank-Wolfe with the Bregman step on the D-optimal objective: the generic solver
(FW_alg_div_step with lmo_simplex: one func_grad per iteration and one value evaluation per line-search trial) against
D_opt_FW_div_step on the maintained state at refresh = 0, 64, 256, 1024, and D_opt_FW (the same rank-one kernels with
the exact line search) from the same process, at (512,8192) and (2048,32768), seed 12, over 200 iterations after a
warm-up run.  Each specialised run also records its largest deviation in F from the generic run,
max |F - F_generic| / max(1, |F_generic|), over the prefix on which the two Ls traces agree, and that prefix.  A run
of 2000 iterations of the classical step (D_opt_FW_descent_step against FW_alg_descent_step) at each refresh shows what
the re-initialisation buys and costs.

Usage:  python tools/fw_div_rate.py [--out profiles/fw_div_rate.json] [--reps 3]
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

SHAPES = [(512, 8192), (2048, 32768)]
ITERS, WARMUP, SEED = 200, 20, 12
REFRESH = [0, 64, 256, 1024]
LONG = 2000


def timed(fn, reps):
    """it/s of ``fn(iters)``: a warm-up run of WARMUP iterations, then the median, min and max of ``reps`` runs"""
    fn(WARMUP)
    rates, out = [], None
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn(ITERS)
        torch.cuda.synchronize()
        rates.append(len(out[1]) / (time.perf_counter() - t))
    return {"median": round(float(np.median(rates)), 1), "min": round(min(rates), 1), "max": round(max(rates), 1),
            "iterations": len(out[1])}, out


def deviation(F, Ls, Fb, Lsb):
    n = min(len(F), len(Fb))
    bad = np.nonzero(np.abs(Ls[:n] - Lsb[:n]) > 1e-12 * (1 + np.abs(Lsb[:n])))[0]
    k = n if bad.size == 0 else int(bad[0])
    return {"Ls_prefix": k, "max_F_dev": float(np.max(np.abs(F[:k] - Fb[:k]) / np.maximum(1, np.abs(Fb[:k]))))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fw_div_rate.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for m, n in SHAPES:
        f, h, L, x0 = acc.D_opt_design(m, n, randseed=SEED)
        lmo = acc.lmo_simplex()
        row = {"shape": [m, n]}
        base, ref = timed(lambda k: acc.FW_alg_div_step(f, h, L, x0, k, 2.0, lmo, verbose=False), 1)
        row["FW_alg_div_step_it_per_s"] = base
        for r in REFRESH:
            rate, got = timed(lambda k: acc.D_opt_FW_div_step(f, L, x0, k, 2.0, verbose=False, refresh=r), a.reps)
            rate.update(deviation(got[1], got[2], ref[1], ref[2]))
            rate["ratio_to_generic"] = round(rate["median"] / base["median"], 1)
            row["D_opt_FW_div_step_refresh_%d" % r] = rate
        rate, got = timed(lambda k: acc.D_opt_FW_descent_step(f, x0, k, verbose=False), a.reps)
        row["D_opt_FW_descent_step_it_per_s"] = rate
        # what `refresh` is for: the classical step has no line search to absorb the drift of the tracked log det
        t = time.perf_counter()
        long_ref = acc.FW_alg_descent_step(f, h, x0, LONG, lmo, verbose=False)
        row["descent_%d" % LONG] = {"FW_alg_descent_step_it_per_s": round(len(long_ref[1]) / (time.perf_counter() - t), 1)}
        for r in REFRESH:
            t = time.perf_counter()
            got = acc.D_opt_FW_descent_step(f, x0, LONG, verbose=False, refresh=r)
            dt = time.perf_counter() - t
            k = min(len(got[1]), len(long_ref[1]))
            row["descent_%d" % LONG]["refresh_%d" % r] = {
                "it_per_s": round(len(got[1]) / dt, 1), "iterations": len(got[1]),
                "max_F_dev": float(np.max(np.abs(got[1][:k] - long_ref[1][:k]) / np.maximum(1, np.abs(long_ref[1][:k])))),
                "x_dev": float(np.max(np.abs(got[0] - long_ref[0])))}
        rate, got = timed(lambda k: acc.D_opt_FW(f, x0, 0.0, k, verbose=False), a.reps)
        row["D_opt_FW_it_per_s"] = rate
        row["cost_of_an_iteration_relative_to_D_opt_FW"] = round(
            rate["median"] / row["D_opt_FW_div_step_refresh_256"]["median"], 2)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del f
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "method": "wall clock of whole solver runs (verbose=False), D_opt_design seed %d, %d iterations after a "
                     "warm-up run of %d, it/s; the generic solver once, the others %d times (median, min, max)"
                     % (SEED, ITERS, WARMUP, a.reps),
           "shapes": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
