"""What one wait per line-search trial gains (DOptimalObj.one_wait_trials): ABPG_gain in one process
with the switch off and on alternating, 5 rounds after a warm-up of each, median and min-max iterations/s per shape.
The traces of the two settings must be equal bit for bit, and at the small shapes the median with the switch on must
not lie below the minimum of the off runs (`on_median_not_below_off_min`).

Usage:  python tools/trial_rate.py [--out FILE.json] [--rounds 5]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

CASES = [(2048, 32768, 40), (512, 8192, 200), (300, 3000, 300)]


def one_run(f, h, x0, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = acc.ABPG_gain(f, h, 1.0, x0, gamma=2, maxitrs=iters, verbose=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return len(out[1]) / dt, out


def case(m, n, iters, rounds):
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    f = acc.DOptimalObj(V)
    h = acc.BurgEntropySimplex()
    x0 = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    rates = {False: [], True: []}
    trace, trials = {}, {}
    for on in (False, True):                                    # warm-up of each
        f.one_wait_trials(on)
        one_run(f, h, x0, iters)
    for _ in range(rounds):
        for on in (False, True):
            f.one_wait_trials(on)
            t0 = f.one_wait_trials_run
            rate, out = one_run(f, h, x0, iters)
            rates[on].append(rate)
            trace[on] = out
            trials[on] = f.one_wait_trials_run - t0
    same = all(bool(torch.equal(a, b)) if isinstance(a, torch.Tensor) else bool(np.array_equal(a, b))
               for a, b in zip(trace[False][:-1], trace[True][:-1]))
    off, on = np.array(rates[False]), np.array(rates[True])
    its = len(trace[True][1])
    return {"shape": [m, n], "iterations": int(its), "trials_per_iteration": trials[True] / its,
            "off_it_per_s": {"median": float(np.median(off)), "min": float(off.min()), "max": float(off.max())},
            "on_it_per_s": {"median": float(np.median(on)), "min": float(on.min()), "max": float(on.max())},
            "ratio_on_over_off": float(np.median(on) / np.median(off)),
            "ms_per_trial_saved": float(1e3 * (1 / np.median(off) - 1 / np.median(on)) * its / max(1, trials[True])),
            "on_median_not_below_off_min": bool(np.median(on) >= off.min()),
            "traces_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    res = {"tool": "tools/trial_rate.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "cases": [case(m, n, iters, args.rounds) for m, n, iters in CASES]}
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
