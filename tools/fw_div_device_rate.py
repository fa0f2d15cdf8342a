"""Iterations per second of D_opt_FW_div_step (the host inside every iteration) against D_opt_FW_div_step_device with
sync_every = 16, 64, 256 (the line search predicted on the device, the host replaying and checking: DESIGN.md 6h), in
one process, on the same objective -- D_opt_design(m, n, randseed=12), gamma 2, line search on, the settings of
tools/fw_div_rate.py.  Each form is timed --reps times after a warm-up run; the record holds the median and the
min-max spread, the ratio of the medians, and the roll-backs and hand-backs of every timed run.  Every timed device
run is asserted bit-identical (x, F, Ls) to the sequential one.

Acceptance (the rule of DESIGN.md 6b): at (2048,32768) the device median is not below the sequential median by more than
the sequential runs' own min-max spread.

Usage:  python tools/fw_div_device_rate.py [--out profiles/fw_div_device_rate.json] [--reps 5]
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

SHAPES = [(30, 1000, 1000), (100, 10000, 1000), (512, 8192, 500), (2048, 32768, 300)]        # (m, n, iterations)
SYNC = (16, 64, 256)


def timed(fn, reps, ref=None):
    """it/s of ``fn()`` -> (result, stats): median, min, max over ``reps`` runs after one warm-up run"""
    out, _ = fn()
    rates, stats = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out, st = fn()
        torch.cuda.synchronize()
        rates.append(len(out[1]) / (time.perf_counter() - t))
        stats.append(st)
        if ref is not None:
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(out[:3], ref[:3])), "device form differs"
    rec = {"median": round(float(np.median(rates)), 1), "min": round(min(rates), 1), "max": round(max(rates), 1),
           "iterations": len(out[1])}
    if ref is not None:
        rec["rollbacks"] = [s["rollbacks"] for s in stats]
        rec["handed_back"] = [s["handed_back"] for s in stats]
        rec["chunks"] = [s["chunks"] for s in stats]
    return rec, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fw_div_device_rate.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for m, n, iters in SHAPES:
        f, h, L, x0 = acc.D_opt_design(m, n, randseed=12)
        seq, ref = timed(lambda: (acc.D_opt_FW_div_step(f, L, x0, iters, 2.0, verbose=False), None), a.reps)
        row = {"shape": [m, n], "sequential_it_per_s": seq}
        for S in SYNC:
            def device():
                stats = {}
                return acc.D_opt_FW_div_step_device(f, L, x0, iters, 2.0, verbose=False, sync_every=S, stats=stats), stats
            dev, _ = timed(device, a.reps, ref)
            dev["ratio_to_sequential"] = round(dev["median"] / seq["median"], 3)
            row["device_S%d_it_per_s" % S] = dev
        if (m, n) == (2048, 32768):
            floor = seq["median"] - (seq["max"] - seq["min"])
            row["acceptance"] = {"floor_it_per_s": round(floor, 1),
                                 "met": {"S%d" % S: bool(row["device_S%d_it_per_s" % S]["median"] >= floor)
                                         for S in SYNC}}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del f
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "method": "wall clock of whole solver runs (verbose=False), D_opt_design seed 12, gamma 2, line search on, "
                     "refresh 256, %d runs after a warm-up run, it/s; x, F, Ls of every timed device run asserted "
                     "bit-identical to the sequential run; rollbacks / handed_back / chunks per timed run" % a.reps,
           "shapes": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
