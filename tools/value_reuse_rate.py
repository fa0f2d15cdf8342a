"""What the value records of libaccbpg_hip cost and gain (DOptimalObj.reuse_values): every case
runs in one process with reuse off and on alternating, 5 rounds after a warm-up of each, and reports median and min-max
iterations/s.  ABPG_gain repeats f at the accepted point and is answered once per iteration; BPG with line search and
ABPG never repeat a value, so for them the switch may only cost -- their reuse-on median must lie inside the min-max of
their reuse-off runs.  `compares_per_iteration` counts the compare launches (an evaluation at another device address
than the record's costs none).

Usage:  python tools/value_reuse_rate.py [--out FILE.json] [--rounds 5]
Prints one JSON object (and writes it to --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402
from accbpg_and_fw_amd import _lib  # noqa: E402

CASES = [("abpg_gain", 2048, 32768, 40), ("abpg_gain", 512, 8192, 200), ("bpg", 80, 200, 300),
         ("bpg", 512, 8192, 150), ("abpg", 512, 8192, 200)]


def counters(f):
    lib = _lib.load()
    cmp_tot = ans_tot = 0
    for h in f._handles():
        c, a = C.c_int64(0), C.c_int64(0)
        lib.accbpg_dopt_value_reuse_stats(h, C.byref(c), C.byref(a))
        cmp_tot, ans_tot = cmp_tot + c.value, ans_tot + a.value
    return cmp_tot, ans_tot


def one_run(solver, f, h, x0, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    if solver == "abpg_gain":
        out = acc.ABPG_gain(f, h, 1.0, x0, gamma=2, maxitrs=iters, verbose=False)
    elif solver == "abpg":
        out = acc.ABPG(f, h, 1.0, x0, gamma=2.0, maxitrs=iters, verbose=False)
    else:
        out = acc.BPG(f, h, 1.0, x0, maxitrs=iters, epsilon=0, linesearch=True, verbose=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return len(out[1]) / dt, out[1]


def case(solver, m, n, iters, rounds):
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    f = acc.DOptimalObj(V)
    h = acc.BurgEntropySimplex()
    x0 = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    rates = {False: [], True: []}
    per_iter = {}
    trace = {}
    for on in (False, True):                                    # warm-up of each
        f.reuse_values(on)
        one_run(solver, f, h, x0, iters)
    for _ in range(rounds):
        for on in (False, True):
            f.reuse_values(on)
            c0 = counters(f)
            rate, F = one_run(solver, f, h, x0, iters)
            c1 = counters(f)
            rates[on].append(rate)
            per_iter[on] = ((c1[0] - c0[0]) / len(F), (c1[1] - c0[1]) / len(F))
            trace[on] = F
    off, on = np.array(rates[False]), np.array(rates[True])
    rec = {"solver": solver, "shape": [m, n], "iterations": int(len(trace[True])),
           "off_it_per_s": {"median": float(np.median(off)), "min": float(off.min()), "max": float(off.max())},
           "on_it_per_s": {"median": float(np.median(on)), "min": float(on.min()), "max": float(on.max())},
           "ratio_on_over_off": float(np.median(on) / np.median(off)),
           "compares_per_iteration": per_iter[True][0], "answered_per_iteration": per_iter[True][1],
           "F_identical": bool(np.array_equal(trace[False], trace[True]))}
    if solver != "abpg_gain":
        rec["on_median_inside_off_min_max"] = bool(off.min() <= np.median(on) <= off.max())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rec = {"device": torch.cuda.get_device_name(0),
           "method": "one process per file, one objective per case; reuse off / on alternating, %d rounds after one "
                     "warm-up run of each; wall clock around the whole solver call, iterations/s" % a.rounds,
           "cases": [case(*c, a.rounds) for c in CASES]}
    s = json.dumps(rec)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
