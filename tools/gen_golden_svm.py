"""Generate tests/golden/svm.npz and tests/golden/svm_digits.npz by running the real reference: SVM_fun and PolyDiv per
call, the factory svm_digits_ds_divs_ball under a seed, and whole runs of BPG, ABPG, FW_alg_div_step, AIBM and AdaptFGM
on a (96,40) Gaussian instance and on the two-class digits set (360,64).

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference package
is imported read-only through oracle/gen_golden.load_reference (no cvxpy: nothing here calls PolyDiv.prox_map) and
called on seeded inputs; only numbers are written.  The Gaussian matrix is not stored: the tests rebuild it
(tests/svm_numpy.gaussian_instance) and compare the checksum.  The digits features are stored as uint8 with the labels,
so that no test needs scikit-learn.

The gradient depends on A x only through the set {i : y_i (A x)_i < 1}, so whole runs reproduce themselves: each run is
repeated three times with the margins A x perturbed at relative 4e-16 (a stand-in for another summation order), and
`prefix` / `xspread` are stored as tools/gen_golden_inexact.py defines them.  Two conditions are asserted: every stored
run has prefix == len(F), and at every per-call point min_i |y_i (A x)_i - 1| >= 1e-6.

Usage:  python tools/gen_golden_svm.py
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from oracle.gen_golden import load_reference, save  # noqa: E402
import svm_numpy as SN  # noqa: E402
from gen_golden_inexact import agree, printed_L  # noqa: E402

FACTORY_SEED = 3                    # frank_wolfe_wtih_rs/ex_SVM.py:20
LAMDAS = [0.01, 1]
DIGITS_RUN_LAMDA = 0.01


def perturbed(accbpg, f, seed):
    """the reference's SVM_fun with its margins multiplied by 1 + 4e-16*N(0,1), from a generator of its own"""
    rng = np.random.RandomState(seed)

    class Perturbed(accbpg.SVM_fun):
        def _z(self, x):
            z = np.dot(self.A, x)
            return z * (1 + 4e-16 * rng.randn(z.size))

        def hinge_loss(self, x):
            return np.mean(np.maximum(0, 1 - self.y * self._z(x)))

        def subgradient_loss(self, x):
            ind = (self.y * self._z(x) < 1).astype(int)
            return np.mean(ind[:, np.newaxis] * self.y[:, np.newaxis] * self.A, axis=0)

    return Perturbed(f.lamda, f.A, f.y)


def percall(accbpg, out, tag, A, y, radius_of):
    """value / gradient pairs of SVM_fun and PolyDiv at three points of the ball, per lamda"""
    rng = np.random.RandomState(5)
    n = A.shape[1]
    for li, lamda in enumerate(LAMDAS):
        radius = radius_of(lamda)
        f = accbpg.SVM_fun(lamda, A, y)
        h = accbpg.PolyDiv(A, lamda=lamda, radius=radius)
        pts = []
        for p in range(3):
            d = rng.randn(n)
            pts.append(d / np.linalg.norm(d) * radius * (0.2 + 0.3 * p))
        pts = np.array(pts)
        key = "%s_l%d" % (tag, li)
        gap = min(np.min(np.abs(y * np.dot(A, x) - 1)) for x in pts)
        assert gap >= 1e-6, "%s: a margin within %.2e of 1: choose other points" % (key, gap)
        fg = [f.func_grad(x, flag=2) for x in pts]
        out.update({
            key + "_lamda": lamda, key + "_radius": radius, key + "_x": pts, key + "_gap": gap,
            key + "_F": np.array([f.F(x) for x in pts]),
            key + "_hinge": np.array([f.hinge_loss(x) for x in pts]),
            key + "_sub": np.array([f.subgradient_loss(x) for x in pts]),
            key + "_fg_f": np.array([v for v, _ in fg]), key + "_fg_g": np.array([g for _, g in fg]),
            key + "_g1": np.array([f.func_grad(x, flag=1) for x in pts]),
            key + "_f0": np.array([f.func_grad(x, flag=0) for x in pts]),
            key + "_ind": np.array([(y * np.dot(A, x) < 1) for x in pts]),
            key + "_h": np.array([h.h(x) for x in pts]),
            key + "_hgrad": np.array([h.gradient(x) for x in pts]),
            key + "_hdiv": np.array([h.divergence(pts[i], pts[(i + 1) % 3]) for i in range(3)]),
            key + "_DS_mean": h.DS_mean, key + "_DS_mean_quad": h.DS_mean_quad,
        })
        print("%-12s gap %.2e  F %s" % (key, gap, out[key + "_F"]), flush=True)


def measure(accbpg, out, tag, f, poly_h, sq_h, L, x0, radius):
    runs = SN.run_table(accbpg, accbpg.lmo_l2_ball)
    for idx, (name, call) in enumerate(runs.items()):
        key = "%s_%s" % (tag, name)
        buf = io.StringIO()
        np.random.seed(SN.RUN_SEED + idx)
        with contextlib.redirect_stdout(buf):
            x, F, G = call(f, poly_h, sq_h, L, np.copy(x0), radius)
        ks, Lk = printed_L(buf.getvalue(), 2)
        assert np.all(np.isfinite(F)) and np.all(np.isfinite(G)) and np.all(np.isfinite(Lk)), key
        prefix, xspread = len(F), 0.0
        for s in range(3):
            np.random.seed(SN.RUN_SEED + idx)
            with contextlib.redirect_stdout(io.StringIO()) as pb:
                xp, Fp, Gp = call(perturbed(accbpg, f, 31 + s), poly_h, sq_h, L, np.copy(x0), radius)
            _, Lp = printed_L(pb.getvalue(), 2)
            assert len(Fp) == len(F), "%s: a perturbed rerun has another length: change the seed" % key
            assert len(Lp) == len(Lk), "%s: a perturbed rerun prints another number of rows" % key
            pre_L = agree(Lp, Lk, 1e-12)            # (a solver may leave its last iteration unprinted)
            pre = min(agree(Fp, F, 1e-9), agree(Gp, G, 1e-12), len(F) if pre_L == len(Lk) else pre_L + int(ks[0]))
            prefix = min(prefix, pre)
            xspread = max(xspread, float(np.max(np.abs(xp - x))))
        assert prefix == len(F), "%s reproduces itself on %d of %d iterations only: change the seed" % (
            key, prefix, len(F))
        out.update({key + "_x": x, key + "_F": F, key + "_G": G, key + "_Lk": Lk, key + "_k0": int(ks[0]),
                    key + "_prefix": prefix, key + "_xspread": xspread})
        print("%-18s len %3d prefix %3d xspread %.2e  F %.6e -> %.6e" % (key, len(F), prefix, xspread, F[0], F[-1]),
              flush=True)


def main():
    accbpg = load_reference()
    import accbpg.utils as U
    from sklearn.datasets import load_digits
    out = {}

    # the digits set as the factory loads it
    X, Y = load_digits(n_class=2, return_X_y=True)
    Y = (Y > 0).astype(int) * 2 - 1
    assert np.array_equal(X, np.round(X)) and X.min() >= 0 and X.max() <= 255
    save("svm_digits", X=X.astype(np.uint8), Y=Y.astype(np.int8))

    # the factory under a seed, per lamda
    for li, lamda in enumerate(LAMDAS):
        np.random.seed(FACTORY_SEED)
        f, (poly_h, sq_h), L, x0, radius = accbpg.svm_digits_ds_divs_ball(lamda=lamda, real_ds=True)
        assert np.array_equal(f.A, X.astype(np.float64)) and np.array_equal(f.y, Y)
        out.update({"fac_l%d_lamda" % li: lamda, "fac_l%d_L" % li: L, "fac_l%d_radius" % li: radius,
                    "fac_l%d_x0" % li: x0, "fac_l%d_DS_mean" % li: poly_h.DS_mean,
                    "fac_l%d_DS_mean_quad" % li: poly_h.DS_mean_quad, "fac_l%d_after" % li: np.random.random_sample()})

    # the utils under a seed
    np.random.seed(7)
    out["u_point"] = U.random_point_in_l2_ball(np.arange(9.0), 2.5)
    out["u_point_pos"] = U.random_point_in_l2_ball(np.zeros(6), 0.5, pos_dir=True)
    out["u_after"] = np.random.random_sample()

    def radius_digits(lamda):
        n = X.shape[1]
        return min(n ** -1 * lamda ** -1 * np.sum(np.linalg.norm(X[:, :-1], axis=1)), (2 / lamda) ** 0.5)

    Xd = X.astype(np.float64)
    percall(accbpg, out, "pc_digits", Xd, Y, radius_digits)

    A, y = SN.gaussian_instance()
    out["gauss_A_checksum"] = np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()])
    out["gauss_y"] = y

    def radius_gauss(lamda):
        n = A.shape[1]
        return min(n ** -1 * lamda ** -1 * np.sum(np.linalg.norm(A[:, :-1], axis=1)), (2 / lamda) ** 0.5)

    percall(accbpg, out, "pc_gauss", A, y, radius_gauss)

    # whole runs
    for tag, M, lab, lamda in (("run_gauss", A, y, SN.GAUSS["lamda"]), ("run_digits", Xd, Y, DIGITS_RUN_LAMDA)):
        np.random.seed(FACTORY_SEED)
        radius, ds_mean, ds_mean_quad, L, x0 = SN.ball_numbers(M, lab, lamda)
        f = accbpg.SVM_fun(lamda, M, lab)
        poly_h, sq_h = accbpg.PolyDiv(M, lamda=lamda, radius=radius), accbpg.SquaredL2Norm()
        assert poly_h.DS_mean == ds_mean and poly_h.DS_mean_quad == ds_mean_quad
        out.update({tag + "_lamda": lamda, tag + "_L": L, tag + "_radius": radius, tag + "_x0": x0})
        measure(accbpg, out, tag, f, poly_h, sq_h, L, x0, radius)

    save("svm", **out)


if __name__ == "__main__":
    main()
