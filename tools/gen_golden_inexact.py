"""Generate tests/golden/inexact.npz by running the real reference: AIBM, AdaptFGM and UniversalGM on
Poisson_regr_simplex_acc (aibm/ex_Poisson_regr.py), the six solver calls of frank_wolfe_wtih_rs/ex_Poisson_regr.py on
one placement of Poisson_regr_simplex, FW_alg_div_step / FW_alg_descent_step with lmo_l2_ball_positive_orthant on
Poisson_regrL2 (parameters_free_fw/ipynb/ex_Poisson_linear_Full_Adapt_and_descent_step.ipynb), the helpers of
accbpg/utils.py:252-295 and per-call outputs of the LMO.

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference package
is imported read-only through oracle/gen_golden.load_reference and called on seeded inputs; only numbers (and the
printed table lines) are written.  A is not stored: the tests rebuild it with the legacy NumPy RNG call sequence of
the factories (accbpg/applications.py:209-295) and compare the checksum.

Not every run is digit-stable, so each run's own spread is measured: the reference is rerun three times with its
value and gradient perturbed at relative 1e-15 (a stand-in for a changed summation order).  Stored per run:
`prefix`, the shortest prefix over the three reruns on which F agrees to 1e-9 and G (and the printed L) to 1e-12, and
`xspread`, the largest |x - x_rerun| (meaningful where the whole run agrees, flag `whole`).

Usage:  python tools/gen_golden_inexact.py        (several minutes)
"""
import contextlib
import io
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from oracle.gen_golden import load_reference, save  # noqa: E402

SEED = 7
ACC = dict(m=2000, n=1000, noise=0.001)         # the drivers' size
ACC_ITERS = 80
FW = dict(m=300, n=500, noise=0.001)
FW_ITERS = 120
FW_PLACE = 'x0_edge_sol_center'
L2 = dict(m=300, n=500, noise=0.001, lamda=0.01, randseed=SEED, normalizeA=True)
L2_ITERS = 120
RUN_SEED = 1991                                 # np.random.seed(RUN_SEED + index) right before each solver call
NOISES = [0, 1e-6]
GAMMAS = [2.0, 1.4, 1.1]


class Perturbed:
    """The reference's f with value and gradient multiplied by 1 + 1e-15*N(0,1), from a generator of its own (the
    global one, which the solvers draw from, is not touched)."""

    def __init__(self, f, seed):
        self.f, self.rng = f, np.random.RandomState(seed)
        self.A, self.b, self.m, self.n = f.A, f.b, f.m, f.n

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def func_grad(self, x, flag=2):
        if flag == 0:
            return self.f(x) * (1 + 1e-15 * self.rng.randn())
        if flag == 1:
            g = self.f.gradient(x)
            return g * (1 + 1e-15 * self.rng.randn(g.size))
        v, g = self.f.func_grad(x, flag=2)
        return v * (1 + 1e-15 * self.rng.randn()), g * (1 + 1e-15 * self.rng.randn(g.size))


def printed_L(text, col):
    """the k and the L column of a printed table"""
    rows = [ln.split() for ln in text.splitlines() if ln[:6].strip().isdigit()]
    return np.array([int(r[0]) for r in rows]), np.array([float(r[col]) for r in rows])


def agree(a, b, tol):
    n = min(len(a), len(b))
    bad = np.nonzero(~(np.abs(a[:n] - b[:n]) <= tol * (1 + np.abs(b[:n]))))[0]
    return n if bad.size == 0 else int(bad[0])


def acc_runs(accbpg):
    """name -> callable(f, h, L, x0) -> (x, F, G) of the ten inexact-oracle runs"""
    runs = {}
    for ni, noise in enumerate(NOISES):
        for gamma in GAMMAS:
            runs["aibm_g%02d_n%d" % (round(gamma * 10), ni)] = \
                lambda f, h, L, x0, gamma=gamma, noise=noise: accbpg.AIBM(f, h, L, x0, gamma=gamma, maxitrs=ACC_ITERS,
                                                                          noise=noise)[:3]
        runs["fgm_n%d" % ni] = lambda f, h, L, x0, noise=noise: accbpg.AdaptFGM(f, h, L, x0, maxitrs=ACC_ITERS,
                                                                                noise=noise)[:3]
        runs["ugm_n%d" % ni] = lambda f, h, L, x0, noise=noise: accbpg.UniversalGM(f, h, L, x0, maxitrs=ACC_ITERS,
                                                                                   noise_level=noise)[:3]
    return runs


def fw_runs(accbpg):
    """the six calls of frank_wolfe_wtih_rs/ex_Poisson_regr.py:25-33 -> (x, F, second trace)"""
    N = FW_ITERS
    return {
        "fw": lambda f, h, L, x0: accbpg.FW_alg_div_step(f, h, L, x0, lmo=accbpg.lmo_simplex(1), maxitrs=N, gamma=2.0,
                                                         ls_ratio=1.5)[:3],
        "bpg": lambda f, h, L, x0: accbpg.BPG(f, h, L, x0, maxitrs=N, linesearch=False)[:3],
        "bpgls": lambda f, h, L, x0: accbpg.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5)[:3],
        "abpg": lambda f, h, L, x0: accbpg.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=False)[:3],
        "expo": lambda f, h, L, x0: (lambda r: (r[0], r[1], r[3]))(
            accbpg.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=N, theta_eq=False, Gmargin=1)),
        "gain": lambda f, h, L, x0: accbpg.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, ls_inc=1.5, ls_dec=1.5,
                                                     theta_eq=True)[:3],
    }


def l2_runs(accbpg):
    """FW_alg_div_step and FW_alg_descent_step with the new LMO, as the notebook calls them"""
    lmo = accbpg.lmo_l2_ball_positive_orthant(1, epsilon=1e-7)
    return {
        "l2div": lambda f, h, L, x0: accbpg.FW_alg_div_step(f, h, L, x0, maxitrs=L2_ITERS, gamma=2.0, lmo=lmo)[:3],
        "l2desc": lambda f, h, L, x0: (lambda r: (r[0], r[1], r[3]))(
            accbpg.FW_alg_descent_step(f, h, x0, maxitrs=L2_ITERS, lmo=lmo)),
    }


def measure(out, tag, runs, f, h, L, x0):
    for idx, (name, call) in enumerate(runs.items()):
        key = "%s_%s" % (tag, name)
        buf = io.StringIO()
        np.random.seed(RUN_SEED + idx)
        with contextlib.redirect_stdout(buf):
            x, F, G = call(f, h, L, np.copy(x0))
        after = np.random.random_sample()
        draws = -1
        for cnt in range(0, 4 * len(F) + 8):                    # how many draws the call made from the global generator
            np.random.seed(RUN_SEED + idx)
            if cnt:
                np.random.random_sample(cnt)
            if np.random.random_sample() == after:
                draws = cnt
                break
        ks, Lk = printed_L(buf.getvalue(), 2)
        assert np.all(np.isfinite(F)) and np.all(np.isfinite(G)) and np.all(np.isfinite(Lk)), key
        prefix, xspread, whole = len(F), 0.0, True
        for s in range(3):
            np.random.seed(RUN_SEED + idx)
            with contextlib.redirect_stdout(io.StringIO()) as pb:
                xp, Fp, Gp = call(Perturbed(f, 31 + s), h, L, np.copy(x0))
            _, Lp = printed_L(pb.getvalue(), 2)
            pre = min(agree(Fp, F, 1e-9), agree(Gp, G, 1e-12), agree(Lp, Lk, 1e-12) + int(ks[0]))
            whole = whole and len(Fp) == len(F) and pre == len(F)
            prefix = min(prefix, pre)
            xspread = max(xspread, float(np.max(np.abs(xp - x))))
        assert prefix >= 60, "%s reproduces itself on %d iterations only: choose another instance" % (key, prefix)
        lines = buf.getvalue().splitlines()
        out.update({key + "_x": x, key + "_F": F, key + "_G": G, key + "_Lk": Lk, key + "_k0": int(ks[0]),
                    key + "_after": after, key + "_draws": draws, key + "_prefix": prefix, key + "_xspread": xspread,
                    key + "_whole": whole, key + "_head": np.array(lines[1:3]), key + "_row": np.array(lines[3])})
        print("%-16s len %3d prefix %3d whole %d xspread %.2e draws %d  L %.3e..%.3e" % (
            key, len(F), prefix, whole, xspread, draws, Lk.min(), Lk.max()), flush=True)


def main():
    accbpg = load_reference()
    out = {}

    # helpers under a seed (the reference keeps three of the four in accbpg.utils only)
    import accbpg.utils as U
    np.random.seed(SEED)
    out["h_rand_point"] = U.random_point_on_simplex(17)
    out["h_rand_point_r2"] = U.random_point_on_simplex(9, radius=2)
    out["h_center_point"] = U.random_point_on_simplex(5, center=True)
    out["h_edge_point"] = U.edge_point_on_simplex(3, 8)
    out["h_edge_point_r2"] = U.edge_point_on_simplex(0, 6, radius=2, tol=1e-3)
    out["h_float"] = np.array([U.get_random_float(0.5), U.get_random_float(0), U.get_random_float()])
    out["h_vector"] = U.get_random_vector(6, 0.25)
    out["h_vector0"] = U.get_random_vector(4, 0)
    out["h_after"] = np.random.random_sample()

    # LMO per call
    rng = np.random.RandomState(5)
    for n in (1, 2, 63, 64, 65, 1000):
        g = rng.randn(n)
        g[0] = -abs(g[0])
        c = rng.rand(n)
        out["lmo_g_%d" % n] = g
        out["lmo_c_%d" % n] = c
        out["lmo_s0_%d" % n] = accbpg.lmo_l2_ball_positive_orthant(1)(g)
        out["lmo_s1_%d" % n] = accbpg.lmo_l2_ball_positive_orthant(0.7, center=c, epsilon=1e-7)(g)
        out["lmo_s2_%d" % n] = accbpg.lmo_l2_ball_positive_orthant(2.0, center=c + 0.5, epsilon=0.0)(g)
        out["lmo_pos_%d" % n] = accbpg.lmo_l2_ball_positive_orthant(1.5, center=c - 0.5, epsilon=1e-3)(np.abs(g))

    # the inexact-oracle methods at the drivers' size
    np.random.seed(SEED)
    f, hs, L, x0 = accbpg.Poisson_regr_simplex_acc(**ACC)
    out["acc_A_checksum"] = np.array([f.A.sum(), np.abs(f.A).max(), (f.A ** 2).sum()])
    out.update({"acc_b": f.b, "acc_L": L, "acc_x0": x0})
    measure(out, "acc", acc_runs(accbpg), f, hs[0], L, x0)

    # the four placements, and the Frank-Wolfe driver's six calls on one of them
    np.random.seed(SEED)
    h, places = accbpg.Poisson_regr_simplex(**FW)
    for key, (fk, Lk, sol, x0k) in places.items():
        out["fw_%s_A_checksum" % key] = np.array([fk.A.sum(), np.abs(fk.A).max(), (fk.A ** 2).sum()])
        out.update({"fw_%s_b" % key: fk.b, "fw_%s_L" % key: Lk, "fw_%s_x0" % key: x0k, "fw_%s_sol" % key: sol})
    fk, Lk, sol, x0k = places[FW_PLACE]
    measure(out, "fw", fw_runs(accbpg), fk, h, Lk, x0k)

    # the new LMO inside the two Frank-Wolfe solvers
    f2, h2, L2c, x02 = accbpg.Poisson_regrL2(**L2)
    out["l2_b"] = f2.b
    measure(out, "l2", l2_runs(accbpg), f2, h2, L2c, x02)

    save("inexact", **out)


if __name__ == "__main__":
    main()
