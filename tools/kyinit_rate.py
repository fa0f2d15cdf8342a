"""Wall seconds of the Kumar-Yildirim start with the host inside every step (D_opt_KYinit) against the form that runs all
m steps on the device (D_opt_KYinit_device), in one process, on the same objective and the same seed of the legacy
generator, and beside them the wall time of 1000 D_opt_FW_away_device iterations from that start -- what the start is
the prelude to.  Per size: the device form is timed --reps times after a warm-up run, the host form likewise except at
the largest size, where it runs once (after the smaller sizes have loaded every kernel it uses); whether the two starts
are array-equal, and if they are not, the smallest relative top-two gap over the host form's arg-extremum decisions
(a difference is expected only where a decision is within rounding of a tie).

Usage:  python tools/kyinit_rate.py [--out profiles/kyinit_rate.json] [--reps 3]
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

SHAPES = [(128, 2048), (512, 8192), (2048, 32768)]
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


def smallest_gap(obj):
    """D_opt_KYinit's own steps (np.dot coefficients, the device's pass over V) with the smallest relative gap between
    the two largest and between the two smallest entries of q^T V over all steps"""
    m = obj.m
    np.random.seed(SEED)
    Q = np.zeros((m, m))
    gap = np.inf
    for i in range(m):
        b = np.random.rand(m)
        q = np.copy(b)
        for j in range(i):
            q = q - np.dot(Q[:, j], b) * Q[:, j]
        w = obj.vt_times(q).cpu().numpy()
        top = np.partition(w, (0, 1, w.size - 2, w.size - 1))
        gap = min(gap, (top[-1] - top[-2]) / np.max(np.abs(w)), (top[1] - top[0]) / np.max(np.abs(w)))
        v = obj.column(int(np.argmin(w))) - obj.column(int(np.argmax(w)))
        q = np.copy(v)
        for j in range(i):
            q = q - np.dot(Q[:, j], v) * Q[:, j]
        Q[:, i] = q / np.linalg.norm(q)
    return float(gap)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kyinit_rate.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rows = []
    for m, n in SHAPES:
        f, h, L, xc = acc.D_opt_design(m, n, randseed=10)
        last = (m, n) == SHAPES[-1]
        wall(lambda: acc.D_opt_KYinit_device(f))                # warm-up
        dev = [wall(lambda: acc.D_opt_KYinit_device(f)) for _ in range(a.reps)]
        x_dev = dev[0][1]
        assert all(np.array_equal(x, x_dev) for _, x in dev), "device start differs between runs"
        if not last:
            wall(lambda: acc.D_opt_KYinit(f))
        host = [wall(lambda: acc.D_opt_KYinit(f)) for _ in range(1 if last else a.reps)]
        x_host = host[0][1]
        equal = bool(np.array_equal(x_dev, x_host))
        run_fw = lambda: acc.D_opt_FW_away_device(f, x_dev, 0.0, FW_ITERS, verbose=False)   # noqa: E731
        out = wall(run_fw)[1]
        assert len(out[1]) == FW_ITERS, len(out[1])
        fw = [wall(run_fw)[0] for _ in range(a.reps)]
        row = {"shape": [m, n], "host_s": spread([t for t, _ in host]), "device_s": spread([t for t, _ in dev]),
               "host_over_device": round(float(np.median([t for t, _ in host]) / np.median([t for t, _ in dev])), 2),
               "fw_away_device_%d_iterations_s" % FW_ITERS: spread(fw),
               "starts_array_equal": equal, "support": int(np.count_nonzero(x_dev)),
               "smallest_decision_gap": None if equal else smallest_gap(f)}
        if last:
            row["device_faster_than_host"] = bool(row["device_s"]["median"] < row["host_s"]["median"])
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
        del f
        torch.cuda.empty_cache()
    rec = {"device": torch.cuda.get_device_name(0), "rocm": torch.version.hip, "torch": torch.__version__,
           "host": {"python": platform.python_version(), "machine": platform.machine()},
           "method": "wall clock around whole calls ending in a device synchronise, np.random.seed(%d) before each, "
                     "D_opt_design(m, n, randseed=10); device form: %d runs after a warm-up run; host form: the same, "
                     "at the largest size one run" % (SEED, a.reps),
           "shapes": rows}
    text = json.dumps(rec, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
