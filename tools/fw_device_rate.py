"""Iterations per second of the Frank-Wolfe D-optimal solvers with the host inside every iteration (D_opt_FW,
D_opt_FW_away) against the forms that decide their steps on the device (D_opt_FW_device with sync_every = 16, 64, 256;
D_opt_FW_away_device at the default R = 16), in one process, on the same objective, for the same fixed number of
iterations (eps = 0: the stop test never holds).  Each form is timed --reps times after a warm-up run; the record
holds the median and the min-max spread, the ratio of the medians, and one probe round trip (launch, synchronise,
read the record) at that shape, which is what the sequential forms pay per iteration on top of their kernels.

Usage:  python tools/fw_device_rate.py [--out profiles/fw_device_rate.json] [--reps 5]
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
from accbpg_and_fw_amd.D_opt_alg import _FWState  # noqa: E402

SHAPES = [(30, 1000, 2000), (100, 10000, 2000), (512, 8192, 1000), (2048, 32768, 500)]      # (m, n, iterations)


def timed(fn, iters, reps):
    """it/s of ``fn()`` (a whole solver run of ``iters`` iterations): median, min, max over ``reps`` runs after one"""
    out = fn()
    assert len(out[1]) == iters, (len(out[1]), iters)
    rates = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        rates.append(iters / (time.perf_counter() - t))
    return {"median": round(float(np.median(rates)), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}, out


def probe_round_trip_us(obj, x0, away):
    st = _FWState(obj, x0)
    for _ in range(20):
        st.probe(away, 0)
    t = time.perf_counter()
    for _ in range(200):
        st.probe(away, 0)
    return round((time.perf_counter() - t) / 200 * 1e6, 2)


def sync_only_us():
    """an empty stream synchronisation, as tools/sync_latency.py times it ("torch sync only")"""
    for _ in range(50):
        torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(2000):
        torch.cuda.synchronize()
    return round((time.perf_counter() - t) / 2000 * 1e6, 2)


def acceptance(row):
    """At (2048,32768), where the pass over V dominates: the device form's median is not below the sequential median
    by more than the sequential runs' own min-max spread."""
    out = {}
    for name, seq, devs in (("fw", row["fw"]["sequential_it_per_s"],
                             {k: v for k, v in row["fw"].items() if k.startswith("device_")}),
                            ("away_R16", row["away_R16"]["sequential_it_per_s"],
                             {"device_it_per_s": row["away_R16"]["device_it_per_s"]})):
        floor = seq["median"] - (seq["max"] - seq["min"])
        out[name] = {"floor_it_per_s": round(floor, 1),
                     "met": {k: bool(v["median"] >= floor) for k, v in devs.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fw_device_rate.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    sync_us = sync_only_us()
    for m, n, iters in SHAPES:
        f, h, L, x0 = acc.D_opt_design(m, n, randseed=10)
        row = {"shape": [m, n], "iterations": iters, "probe_round_trip_us": probe_round_trip_us(f, x0, 0)}
        seq, ref = timed(lambda: acc.D_opt_FW(f, x0, 0.0, iters, verbose=False), iters, a.reps)
        row["fw"] = {"sequential_it_per_s": seq}
        for S in (16, 64, 256):
            dev, got = timed(lambda: acc.D_opt_FW_device(f, x0, 0.0, iters, verbose=False, sync_every=S), iters, a.reps)
            assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(got[:4], ref[:4])), "device form differs"
            dev["ratio_to_sequential"] = round(dev["median"] / seq["median"], 3)
            row["fw"]["device_S%d_it_per_s" % S] = dev
        seq, ref = timed(lambda: acc.D_opt_FW_away(f, x0, 0.0, iters, verbose=False), iters, a.reps)
        dev, got = timed(lambda: acc.D_opt_FW_away_device(f, x0, 0.0, iters, verbose=False), iters, a.reps)
        assert all(np.array_equal(p, q, equal_nan=True) for p, q in zip(got[:4], ref[:4])), "device form differs"
        dev["ratio_to_sequential"] = round(dev["median"] / seq["median"], 3)
        row["away_R16"] = {"sequential_it_per_s": seq, "device_it_per_s": dev}
        if (m, n) == (2048, 32768):
            row["acceptance"] = acceptance(row)
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del f
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "method": "wall clock of whole solver runs (verbose=False, eps=0), %d runs after a warm-up run, it/s; "
                     "x, F, SP, SN of every device form asserted bit-identical to the sequential run" % a.reps,
           "sync_only_us": sync_us, "shapes": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
