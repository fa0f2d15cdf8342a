"""The lock-step Bregman-step batch that predicts its steps on the device (D_opt_FW_div_step_batch_device)
against the two routes that existed before it, on the same instances in one process:

  batch          D_opt_FW_div_step_batch on a DOptimalBatch: one synchronisation per lock-step iteration
  device_loop    D_opt_FW_div_step_device(batch.instance(i), ...) for i = 0 .. K-1, one after the other
  python_S, c_S  D_opt_FW_div_step_batch_device with replay "python" / "c" and sync_every = S, S = 16 and 64

The matrices are those of D_opt_design(m, n, randseed=11+i); L = 1, gamma = 2, line search on, the default refresh,
200 iterations from the uniform start.  Every run is a whole solve of all K instances timed by the wall clock
(initialisation included; the batch and its handles are built before the clock starts); one warm-up and five runs per
route, the routes alternating, reported as median (min - max) of instance-iterations per second, with the roll-backs and
hand-backs per run.  Every device_loop, python_S and c_S run is asserted bit-identical (x, F, Ls, iteration count) to the
batch run beside it.  The cost of the per-chunk snapshot is timed alone at the end of each case.

The gates are the project's own: at (512,8192) x 64 the new form "pays" only if the median of c_64 or c_16 exceeds the
batch route's median by more than the batch route's own min-max spread; at (2048,32768) x 4 parity means not below that
median by more than that spread.

Usage:  python tools/fw_div_batch_device_rate.py [--out profiles/fw_div_batch_device_rate.json] [--iters 200] [--runs 5]
                                                 [--cases 30x1000x64,512x8192x8,512x8192x64,2048x32768x4]
Prints one JSON object (and writes it to --out)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=200)
ap.add_argument("--runs", type=int, default=5)
ap.add_argument("--cases", default="30x1000x64,512x8192x8,512x8192x64,2048x32768x4")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

SYNCS = (16, 64)


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(rates):
    return {"median": round(statistics.median(rates), 1), "min": round(min(rates), 1), "max": round(max(rates), 1)}


def identical(res, ref, what):
    for i, (a, b) in enumerate(zip(res, ref)):
        assert len(a[1]) == len(b[1]), "%s: instance %d ran %d iterations, the batch route %d" % (what, i, len(a[1]), len(b[1]))
        for name, u, v in zip(("x", "F", "Ls"), a[:3], b[:3]):
            assert np.array_equal(np.asarray(u).view(np.int64), np.asarray(v).view(np.int64)), \
                "%s: instance %d: %s differs from the batch route" % (what, i, name)


def case(m, n, K, iters, runs):
    Vs = []
    for i in range(K):
        np.random.seed(11 + i)                                   # the matrix of D_opt_design(m, n, randseed=11+i)
        Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    routes = {"batch": lambda st: acc.D_opt_FW_div_step_batch(batch, 1.0, x0, iters, 2.0)}

    def device_loop(st):
        out = []
        for i in range(K):
            one = {}
            out.append(acc.D_opt_FW_div_step_device(batch.instance(i), 1.0, x0, iters, 2.0, verbose=False, stats=one))
            for key, v in one.items():
                st[key] = st.get(key, 0) + v
        return out
    routes["device_loop"] = device_loop
    for S in SYNCS:
        for replay in ("python", "c"):
            routes["%s_%d" % (replay, S)] = (lambda st, S=S, replay=replay: acc.D_opt_FW_div_step_batch_device(
                batch, 1.0, x0, iters, 2.0, sync_every=S, stats=st, replay=replay))
    rates = {name: [] for name in routes}
    events = {name: {"rollbacks": [], "handed_back": []} for name in routes if name != "batch"}
    for run in range(runs + 1):                                 # (run 0 is the warm-up)
        ref = None
        for name, fn in routes.items():
            st = {}
            dt, res = timed(lambda: fn(st))
            if name == "batch":
                ref = res
            else:
                identical(res, ref, name)
            if run:
                rates[name].append(sum(len(r[1]) for r in res) / dt)
                if name != "batch":
                    for key in events[name]:
                        events[name][key].append(int(st.get(key, 0)))
    rec = {"shape": [m, n], "K": K, "iters": iters, "iterations_run": [len(r[1]) for r in ref],
           "bit_identical_to_batch": True}
    for name in routes:
        rec[name] = spread(rates[name])
        if name != "batch":
            rec[name].update({key + "_per_run": v for key, v in events[name].items()})
            rec[name]["over_batch_median"] = round(rec[name]["median"] / rec["batch"]["median"], 3)
    rec["batch_min_max_spread"] = round(rec["batch"]["max"] - rec["batch"]["min"], 1)
    best = max(("c_%d" % S for S in SYNCS), key=lambda name: rec[name]["median"])
    rec["best_c"] = best
    rec["best_c_median_minus_batch_median"] = round(rec[best]["median"] - rec["batch"]["median"], 1)
    rec["pays"] = bool(rec["best_c_median_minus_batch_median"] > rec["batch_min_max_spread"])
    rec["parity"] = bool(rec["best_c_median_minus_batch_median"] >= -rec["batch_min_max_spread"])
    snaps = [timed(lambda: batch.fw_snapshot(None))[0] for _ in range(6)][1:]
    rec["snapshot_all_instances_ms"] = spread([1e3 * s for s in snaps])
    return rec


def main():
    cases = []
    for spec in ARGS.cases.split(","):
        m, n, K = (int(v) for v in spec.split("x"))
        cases.append(case(m, n, K, ARGS.iters, ARGS.runs))
        torch.cuda.empty_cache()
    rec = {
        "device": torch.cuda.get_device_name(0), "unit": "instance-iterations per second", "runs": ARGS.runs,
        "cases": cases,
        "method": "wall clock around the whole solve of all K instances (initialisation included; one warm-up run per "
                  "route, not counted), D_opt_design(m, n, randseed=11+i), L = 1, gamma = 2, line search on, default "
                  "refresh, uniform x0; batch = D_opt_FW_div_step_batch, device_loop = D_opt_FW_div_step_device on "
                  "batch.instance(i) one after the other, python_S / c_S = D_opt_FW_div_step_batch_device with that "
                  "replay and sync_every = S; the routes alternate inside every run; median / min / max over the runs; "
                  "every run of every other route asserted bit-identical (x, F, Ls, iteration count) to the batch run "
                  "beside it; pays: best c median above the batch median by more than the batch route's min-max spread; "
                  "parity: not below it by more than that spread; snapshot_all_instances_ms: fw_snapshot of all K "
                  "instances timed alone, five calls",
    }
    s = json.dumps(rec)
    print(s)
    if ARGS.out:
        os.makedirs(os.path.dirname(os.path.abspath(ARGS.out)), exist_ok=True)
        with open(ARGS.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
