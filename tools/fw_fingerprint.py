"""Fingerprints of the eight Frank-Wolfe D-optimal solvers, for comparing two builds of the library bit for bit (the
GPU tests compare the solvers with each other and with NumPy, not one commit with another).

Each solver runs 40 iterations (eps = 0: the stop test never holds) on seeded Gaussian designs at (7, 300), (30, 5000)
and (64, 140000), from the centre of the simplex.  The batch forms take K = 3 matrices with the middle instance
inactive: its eps is infinite, so it stops at its first probe and the later launches cover the active set {0, 2}.  The
single forms run on the first matrix.  The away forms leave ``logdet_refresh`` at its default.  One SHA-256 per solver
and shape is taken over the raw bytes of x, F, SP and SN (of every instance, in order, for a batch).

Usage:  python tools/fw_fingerprint.py [--out fingerprint.json]
Prints one line per solver and shape; two builds agree when their outputs are equal line for line."""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accbpg_and_fw_amd as acc  # noqa: E402

SHAPES = [(7, 300), (30, 5000), (64, 140000)]
ITERS = 40
K = 3
SINGLE = ("D_opt_FW", "D_opt_FW_away", "D_opt_FW_device", "D_opt_FW_away_device")
BATCH = ("D_opt_FW_batch", "D_opt_FW_away_batch", "D_opt_FW_batch_device", "D_opt_FW_away_batch_device")


def digest(results):
    h = hashlib.sha256()
    for res in results:
        for a in res[:4]:                                        # x, F, SP, SN (T is wall-clock time)
            h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    rec = {}
    for m, n in SHAPES:
        Vs = []
        for i in range(K):
            np.random.seed(1000 * m + i + 1)
            Vs.append(torch.from_numpy(np.random.randn(m, n)).cuda())
        x0 = np.ones(n) / n
        batch = acc.DOptimalBatch(Vs)
        eps = [0.0, float("inf"), 0.0]
        for name in SINGLE:
            res = getattr(acc, name)(batch.instance(0), x0, 0.0, ITERS, verbose=False)
            assert len(res[1]) == ITERS, (name, len(res[1]))
            rec["%s %dx%d" % (name, m, n)] = digest([res])
        for name in BATCH:
            res = getattr(acc, name)(batch, x0, eps, ITERS)
            assert [len(r[1]) for r in res] == [ITERS, 1, ITERS], (name, [len(r[1]) for r in res])
            rec["%s %dx%dx%d" % (name, m, n, K)] = digest(res)
        del batch, Vs
        torch.cuda.empty_cache()
    for key, sha in rec.items():
        print("%-40s %s" % (key, sha))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
