"""Extended-precision references of f and g for badly conditioned Gram matrices: tests/golden/ext_*.npz.

Does not use the reference package.  For seeded inputs (V, x) it forms H = V diag(x) V^T, its Cholesky factor L,
W = L^-1 V, f = -2 sum log L_ii and g_j = -||W e_j||^2 entirely in np.longdouble (x87 extended, 64-bit mantissa),
with NumPy's own loops (no BLAS, no LAPACK), and stores f and g rounded to float64 with kappa_2(H) (LAPACK, fp64,
informative only) and SHA-256 checksums of V's and x's bytes.

V is built with the legacy RandomState and elementwise NumPy operations only, so that a test rebuilds it bit for bit
(``make_V`` / ``make_x``; the test asserts the checksums before it uses them):
  graded  row i of a Gaussian matrix times 10^((i mod 7) - 3), taken from a table of literals.  A Cholesky-based
          evaluation is nearly invariant under this row scaling, so fp64 results stay close to the unit roundoff.
  ill     each of the last three rows is the sum of two earlier rows plus eps * (a fresh Gaussian row), eps in
          1e-3, 1e-4, 1e-5: kappa(H) of 1e8 .. 1e11 that no diagonal scaling removes.
x is uniform, or the Kumar-Yildirim-style mixture: 2m entries of 1/(2m) at seeded places, the rest 1e-4/n.

The longdouble Gram runs at about 0.25 GMAC/s, so the (2048, 6144) cases take minutes; the cases run in parallel.

Usage:
    python oracle/gen_extended.py                 # write every fixture
    python oracle/gen_extended.py --check         # recompute and compare f and g with the stored ones bit for bit
    python oracle/gen_extended.py --only NAME ... # a subset
"""
import argparse
import hashlib
import os
import sys
import time

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden")

SCALES = (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3)        # 10^((i mod 7) - 3), literals (no pow: libm may differ)
EPS = (1e-3, 1e-4, 1e-5)

# name: (kind, m, n, seed, x kind).  n > 2m everywhere, so the mixture start is not uniform.
CASES = {
    "ext_graded_1024x4096": ("graded", 1024, 4096, 11, "mixture"),
    "ext_ill_1024x4096_a": ("ill", 1024, 4096, 12, "uniform"),
    "ext_ill_1024x4096_b": ("ill", 1024, 4096, 13, "mixture"),
    "ext_ill_1024x4096_c": ("ill", 1024, 4096, 14, "uniform"),
    "ext_graded_2048x6144": ("graded", 2048, 6144, 15, "uniform"),
    "ext_ill_2048x6144": ("ill", 2048, 6144, 16, "mixture"),
    "ext_graded_1000x3001": ("graded", 1000, 3001, 17, "uniform"),
    "ext_ill_1000x3001": ("ill", 1000, 3001, 18, "mixture"),
}


def make_V(kind, m, n, seed):
    rs = np.random.RandomState(seed)
    V = rs.randn(m, n)
    if kind == "graded":
        for i in range(m):
            V[i] *= SCALES[i % 7]
    elif kind == "ill":
        for k, eps in enumerate(EPS):
            V[m - 3 + k] = (V[2 * k] + V[2 * k + 1]) + eps * rs.randn(n)
    else:
        raise ValueError(kind)
    return V


def make_x(xkind, m, n, seed):
    if xkind == "uniform":
        return np.full(n, 1.0 / n)
    if xkind == "mixture":
        rs = np.random.RandomState(seed + 1000)
        x = np.full(n, 1e-4 / n)
        x[rs.permutation(n)[: 2 * m]] = 1.0 / (2 * m)
        return x
    raise ValueError(xkind)


def inputs(name):
    kind, m, n, seed, xkind = CASES[name]
    return make_V(kind, m, n, seed), make_x(xkind, m, n, seed)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def extended_f_g(V, x):
    """f and g of the D-optimal objective in np.longdouble (NumPy loops only)."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not extended precision on this machine"
    Vl = V.astype(np.longdouble)
    H = np.matmul(Vl * x.astype(np.longdouble), Vl.T)
    m = H.shape[0]
    # right-looking Cholesky, column by column (the trailing update is symmetric: only its lower part is used)
    L = np.zeros_like(H)
    A = H.copy()
    for j in range(m):
        d = A[j, j]
        if not d > 0:
            raise ValueError("not positive definite in extended precision")
        r = np.sqrt(d)
        col = A[j + 1:, j] / r
        L[j, j] = r
        L[j + 1:, j] = col
        A[j + 1:, j + 1:] -= np.outer(col, col)
    # W = L^-1 V, row by row
    W = np.empty_like(Vl)
    for i in range(m):
        W[i] = (Vl[i] - np.matmul(L[i, :i], W[:i])) / L[i, i] if i else Vl[i] / L[i, i]
    f = -2 * np.sum(np.log(np.diagonal(L)))
    g = -np.sum(W * W, axis=0)
    return f, g, H


def compute(name):
    t0 = time.time()
    V, x = inputs(name)
    f, g, H = extended_f_g(V, x)
    kappa = float(np.linalg.cond(H.astype(np.float64)))
    return name, dict(f=np.float64(f), g=g.astype(np.float64), kappa=np.float64(kappa), v_sha256=np.str_(sha(V)),
                      x_sha256=np.str_(sha(x))), time.time() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the stored fixtures instead of writing them")
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    args = ap.parse_args()
    names = args.only or sorted(CASES, key=lambda k: -CASES[k][1] * CASES[k][1] * CASES[k][2])   # longest first
    from concurrent.futures import ProcessPoolExecutor
    bad = 0
    with ProcessPoolExecutor(max_workers=max(1, min(args.jobs, len(names)))) as pool:
        for name, res, secs in pool.map(compute, names):
            path = os.path.join(OUT, name + ".npz")
            if args.check:
                old = np.load(path)
                same = (old["f"].tobytes() == res["f"].tobytes() and old["g"].tobytes() == res["g"].tobytes()
                        and str(old["v_sha256"]) == str(res["v_sha256"]))
                bad += not same
                print("%-24s %s (%.0f s)" % (name, "same" if same else "DIFFERS", secs))
            else:
                np.savez_compressed(path, **res)
                print("wrote %s  kappa=%.2e  f=%.17g  (%.0f s)" % (path, res["kappa"], res["f"], secs))
            sys.stdout.flush()
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
