"""Generate tests/golden/logistic.npz by running the real reference's L2L1Linf, SquaredL2Norm, solvers and
lmo_linf_ball on a NumPy logistic objective.

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference package is
imported read-only through oracle/gen_golden.load_reference and called on seeded inputs; only numbers are written.
The reference's own LogisticRegression class is written in jax, which is a stub here, so it cannot run: the objective
is a NumPy stand-in defined here under the reference's RSmoothFunction protocol, written with library routines of its
own and not with the formulas of tests/logistic_numpy.py: the value is mean(np.logaddexp(0, -s)), the gradient
-(y * scipy.special.expit(-s)) A / m, s = y * (A x).  The goldens are therefore evidence that does not depend on the
restatement; the two agree to rounding, not bit for bit.  Everything else -- L2L1Linf, SquaredL2Norm, BPG, ABPG,
ABPG_gain, ABPG_expo, ABDA, FW_alg_div_step, lmo_linf_ball -- is the real reference's.

Contents: f, g, A x at three points of the box on the (96,40) Gaussian instance with mixed labels (the matrix is
rebuilt by the tests, only its checksum is stored); L2L1Linf's prox_map, div_prox_map, extra_Psi and divergence at
those points for L in {0.05, 40} and lamda in {0, 1/m, 0.3}; whole runs of 100 iterations at the example's shape
(100,200).  Each run is repeated three times with the margins A x perturbed at relative 4e-16 (a stand-in for another
summation order), and `prefix` / `xspread` are stored as tools/gen_golden_inexact.py defines them; every stored run
must have prefix == len(F).

Usage:  python tools/gen_golden_logistic.py
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
import logistic_numpy as LN  # noqa: E402
from gen_golden_inexact import agree, printed_L  # noqa: E402


def stand_in(accbpg, X, y, perturb=None):
    """The NumPy objective as a subclass of the reference's RSmoothFunction.  `perturb` (a RandomState) multiplies the
    margins by 1 + 4e-16*N(0,1), the stand-in for another summation order."""
    from scipy.special import expit

    class Logistic(accbpg.RSmoothFunction):
        def __init__(self):
            self.X, self.y = X, np.asarray(y, dtype=np.float64).reshape(-1)
            self.m, self.n = X.shape

        def _s(self, x):
            z = np.dot(self.X, x)
            if perturb is not None:
                z = z * (1 + 4e-16 * perturb.randn(z.size))
            return self.y * z

        def __call__(self, x):
            return self.func_grad(x, flag=0)

        def gradient(self, x):
            return self.func_grad(x, flag=1)

        def func_grad(self, x, flag=2):
            s = self._s(x)
            f = np.sum(np.logaddexp(0.0, -s)) / self.m
            if flag == 0:
                return f
            g = np.dot(-(self.y * expit(-s)), self.X) / self.m
            return g if flag == 1 else (f, g)

    return Logistic()


def percall(accbpg, out):
    A, y = LN.gaussian_instance()
    m, n = A.shape
    pts = LN.box_points(n)
    f = stand_in(accbpg, A, y)
    fg = [f.func_grad(x, flag=2) for x in pts]
    out.update({"gauss_A_checksum": np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()]), "gauss_y": y, "pc_x": pts,
                "pc_f": np.array([v for v, _ in fg]), "pc_g": np.array([g for _, g in fg]),
                "pc_Ax": np.array([np.dot(A, x) for x in pts])})
    lamdas = [0.0, 1.0 / m, 0.3]
    out["k_lamda"], out["k_L"] = np.array(lamdas), np.array(LN.KERNEL_L)
    shape = (len(lamdas), len(LN.KERNEL_L), 3, n)
    prox, dprox = np.zeros(shape), np.zeros(shape)
    psi, div, hval = np.zeros((len(lamdas), 3)), np.zeros(3), np.zeros(3)
    for a, lamda in enumerate(lamdas):
        h = accbpg.L2L1Linf(lamda=lamda, B=1)
        for i, x in enumerate(pts):
            psi[a, i] = h.extra_Psi(x)
            div[i] = h.divergence(x, pts[(i + 1) % 3])
            hval[i] = h(x)
            for b, L in enumerate(LN.KERNEL_L):
                prox[a, b, i] = h.prox_map(np.copy(fg[i][1]), L)
                dprox[a, b, i] = h.div_prox_map(np.copy(x), np.copy(fg[i][1]), L)
    out.update({"k_prox": prox, "k_dprox": dprox, "k_psi": psi, "k_div": div, "k_h": hval})
    print("per call: f %s" % out["pc_f"], flush=True)


def runs(accbpg, out):
    A, _ = LN.example_draws()
    y = LN.example_labels()
    m, n = A.shape
    B, L, x0 = LN.EXAMPLE["B"], 0.25, np.zeros(n)
    h, sh = accbpg.L2L1Linf(lamda=1.0 / m, B=B), accbpg.SquaredL2Norm()
    out.update({"run_A_checksum": np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()]), "run_y": y, "run_L": L,
                "run_lamda": 1.0 / m, "run_B": B})
    table = LN.run_table(accbpg, accbpg.lmo_linf_ball)
    for idx, (name, call) in enumerate(table.items()):
        key = "run_" + name
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            x, F, G = call(stand_in(accbpg, A, y), h, sh, L, np.copy(x0), B)
        ks, Lk = printed_L(buf.getvalue(), 2)
        assert np.all(np.isfinite(F)) and np.all(np.isfinite(G)) and np.all(np.isfinite(Lk)), key
        prefix, xspread = len(F), 0.0
        for s in range(3):
            with contextlib.redirect_stdout(io.StringIO()) as pb:
                xp, Fp, Gp = call(stand_in(accbpg, A, y, perturb=np.random.RandomState(31 + s)), h, sh, L, np.copy(x0),
                                  B)
            _, Lp = printed_L(pb.getvalue(), 2)
            assert len(Fp) == len(F), "%s: a perturbed rerun has another length: change the seed" % key
            assert len(Lp) == len(Lk), "%s: a perturbed rerun prints another number of rows" % key
            pre_L = agree(Lp, Lk, 1e-12)
            pre = min(agree(Fp, F, 1e-9), agree(Gp, G, 1e-9), len(F) if pre_L == len(Lk) else pre_L + int(ks[0]))
            prefix = min(prefix, pre)
            xspread = max(xspread, float(np.max(np.abs(xp - x))))
        assert prefix == len(F), "%s reproduces itself on %d of %d iterations only: change the seed" % (
            key, prefix, len(F))
        out.update({key + "_x": x, key + "_F": F, key + "_G": G, key + "_Lk": Lk, key + "_k0": int(ks[0]),
                    key + "_prefix": prefix, key + "_xspread": xspread})
        print("%-12s len %3d prefix %3d xspread %.2e  F %.6e -> %.6e" % (key, len(F), prefix, xspread, F[0], F[-1]),
              flush=True)


def main():
    accbpg = load_reference()
    out = {}
    percall(accbpg, out)
    runs(accbpg, out)
    save("logistic", **out)


if __name__ == "__main__":
    main()
