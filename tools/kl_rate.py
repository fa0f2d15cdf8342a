"""KL-divergence regression against the Poisson problem on the same (8192, 65536) matrix, in one process:
KLdivRegression.func_grad against PoissonRegression.func_grad (the two share both passes over A and differ in the
per-row epilogue only), and ABPG with ShannonEntropyL1 on KL against ABPG with BurgEntropyL1 on Poisson.

Usage:  python tools/kl_rate.py [--out FILE.json] [--m 8192] [--n 65536]
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


def fg_times(fs, x, reps, rounds):
    """median ms per func_grad(x, 2) of each objective, interleaved round by round (drift hits both alike)"""
    g = {id(f): [] for f in fs}
    for f in fs:
        for _ in range(3):
            f.func_grad(x, 2)
    for _ in range(rounds):
        for f in fs:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(reps):
                f.func_grad(x, 2)              # returns the value: synchronises every call
            torch.cuda.synchronize()
            g[id(f)].append((time.perf_counter() - t) / reps * 1e3)
    return [float(np.median(g[id(f)])) for f in fs]


def abpg_rate(f, h, L, x0, iters):
    acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=3, theta_eq=True, verbose=False)
    torch.cuda.synchronize()
    t = time.perf_counter()
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=iters, theta_eq=True, verbose=False)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return len(F) / dt, float(F[0]), float(F[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--m", type=int, default=8192)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    m, n = a.m, a.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    A = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=gen)
    A /= A.sum(dim=0)                                            # column sums 1, as the factories normalise
    xt = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen)
    b = A @ xt + 0.01 * (torch.rand(m, dtype=torch.float64, device="cuda", generator=gen) - 0.5)   # plumbing only
    assert float(b.min()) > 0
    fk = acc.KLdivRegression(A, b)
    fp = acc.PoissonRegression(A, b)
    x = torch.full((n,), 0.5, dtype=torch.float64, device="cuda")
    t_kl, t_po = fg_times([fk, fp], x, a.reps, a.rounds)
    bytes_fg = 2 * 8 * m * n
    r_kl = abpg_rate(fk, acc.ShannonEntropyL1(0.001), 1.0, x, a.iters)
    x0p = torch.full((n,), 10.0 / n, dtype=torch.float64, device="cuda")
    r_po = abpg_rate(fp, acc.BurgEntropyL1(0.001), float(b.sum()), x0p, a.iters)
    rec = {
        "device": torch.cuda.get_device_name(0), "shape": [m, n],
        "func_grad_ms": {"kl": round(t_kl, 4), "poisson": round(t_po, 4), "ratio_kl_over_poisson": round(t_kl / t_po, 4)},
        "func_grad_TBps": {"kl": round(bytes_fg / t_kl * 1e-9, 3), "poisson": round(bytes_fg / t_po * 1e-9, 3)},
        "abpg_it_per_s": {"kl_shannonL1": round(r_kl[0], 3), "poisson_burgL1": round(r_po[0], 3),
                          "ratio_kl_over_poisson": round(r_kl[0] / r_po[0], 4)},
        "abpg_F": {"kl": [r_kl[1], r_kl[2]], "poisson": [r_po[1], r_po[2]]},
        "method": "func_grad(x, 2): median over %d interleaved rounds of %d calls each; ABPG(gamma=2, theta_eq=True) "
                  "%d iterations after a 3-iteration warm-up, wall clock" % (a.rounds, a.reps, a.iters),
    }
    s = json.dumps(rec)
    print(s)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(s + "\n")


if __name__ == "__main__":
    main()
