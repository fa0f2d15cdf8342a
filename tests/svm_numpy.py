"""NumPy restatement of the reference's SVM family (accbpg/functions.py:161-194 and 838-905; accbpg/applications.py:
298-327; accbpg/utils.py:161-212), for the CPU tests: it reproduces tests/golden/svm.npz, written by the real reference
(tools/gen_golden_svm.py), and is what the GPU tests compare the device classes with.

PolyDiv.prox_map is the one place where the reference is not restated but solved: the reference states
    min  L*phi(||x||) + <g', x>   over ||x|| <= radius,      g' = g/||g||*radius  (||g|| := 1e-8 when it is 0),
    phi(t) = lamda^2/4 t^4 + 2 lamda DS_mean/3 t^3 + DS_mean_quad/2 t^2
to a conic solver.  For a fixed norm t the linear term is smallest at x = -t g'/||g'|| = -t g/||g||, where it is
-t*radius (0 when g = 0), so the problem is the scalar one  min_{0 <= t <= radius} L*phi(t) - radius*t,  convex because
phi' is increasing on t >= 0:  t* = min(radius, t^) with L*phi'(t^) = radius.  Here the root is found by bisection to
the last bit, independently of the package's safeguarded Newton iteration.

The solver loops come from the restatements the other families use: BPG, ABPG and FW_alg_div_step of
oracle/np_oracle.py, AIBM and AdaptFGM of tests/inexact_numpy.py.  The package does not import this module."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
from oracle.np_oracle import ABPG, BPG, FW_alg_div_step  # noqa: E402,F401
from inexact_numpy import AIBM, AdaptFGM, SquaredL2Norm  # noqa: E402,F401

GOLDEN = os.path.join(_HERE, "golden")

# the Gaussian instance of the goldens: rebuilt from a RandomState of its own, never stored
GAUSS = dict(m=96, n=40, seed=11, lamda=0.1)


def gaussian_instance(m=GAUSS["m"], n=GAUSS["n"], seed=GAUSS["seed"]):
    """(A, y): N(0,1) features, labels from a noisy random hyperplane (so both classes and both sides of the margin
    occur)"""
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n)
    w = rng.randn(n)
    y = np.where(A.dot(w) + 0.5 * rng.randn(m) > 0, 1, -1)
    return A, y


def digits_instance():
    """(X, Y) of the two-class digits set as the reference's factory sees it: float64 features, labels -1 / +1"""
    z = np.load(os.path.join(GOLDEN, "svm_digits.npz"), allow_pickle=False)
    return z["X"].astype(np.float64), z["Y"].astype(np.int64)


class SVM_fun:
    def __init__(self, lamda, A, y):
        self.lamda, self.A, self.y = lamda, A, y

    def __call__(self, x):
        return self.F(x)

    def margins(self, x):
        return np.dot(self.A, x)

    def hinge_loss(self, x):
        return np.mean(np.maximum(0, 1 - self.y * np.dot(self.A, x)))

    def F(self, x):
        return self.hinge_loss(x) + self.lamda / 2 * np.dot(x, x)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def indicator(self, x):
        return self.y * np.dot(self.A, x) < 1

    def subgradient_loss(self, x):
        ind = self.indicator(x).astype(int)
        return np.mean(ind[:, None] * self.y[:, None] * self.A, axis=0)

    def func_grad(self, x, flag=2):
        if flag == 0:
            return self.F(x)
        g = self.lamda * x - self.subgradient_loss(x)
        if flag == 1:
            return g
        return self.F(x), g


def prox_radius(L, lamda, ds_mean, ds_mean_quad, radius):
    """t* = min(radius, t^), L*phi'(t^) = radius, by bisection on [0, radius]"""
    def dphi(t):
        return lamda ** 2 * t ** 3 + 2 * lamda * ds_mean * t ** 2 + ds_mean_quad * t
    if not L * dphi(radius) > radius:
        return float(radius)
    lo, hi = 0.0, float(radius)
    for _ in range(2000):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if L * dphi(mid) > radius:
            hi = mid
        else:
            lo = mid
    return 0.5 * (lo + hi)


class PolyDiv:
    def __init__(self, DS, lamda=0, radius=1):
        self.lamda, self.radius, self.DS = lamda, radius, DS
        self.DS_mean = np.mean(np.linalg.norm(DS, axis=1))
        self.DS_mean_quad = np.mean(np.linalg.norm(DS, axis=1) ** 2)

    def __call__(self, x):
        return self.h(x)

    def h(self, x):
        nrm = np.linalg.norm(x)
        return self.lamda ** 2 * (1 / 4 * nrm ** 4) + 2 * self.lamda * self.DS_mean * (1 / 3 * nrm ** 3) \
            + self.DS_mean_quad * (1 / 2 * nrm ** 2)

    def phi(self, t):
        return self.lamda ** 2 / 4 * t ** 4 + 2 * self.lamda * self.DS_mean / 3 * t ** 3 + self.DS_mean_quad / 2 * t ** 2

    def dphi(self, t):
        return self.lamda ** 2 * t ** 3 + 2 * self.lamda * self.DS_mean * t ** 2 + self.DS_mean_quad * t

    def extra_Psi(self, x):
        return 0

    def gradient(self, x):
        # the reference's factor, lamda**4 included: not the derivative of h
        return (self.lamda ** 4 * np.linalg.norm(x) ** 2 + 2 * self.lamda * self.DS_mean + self.DS_mean_quad) * x

    def divergence(self, x, y):
        assert x.shape == y.shape
        return self.h(x) - self.h(y) - np.dot(self.gradient(y), x - y)

    def scaled(self, g):
        """g' of the stated problem"""
        g_norm = np.linalg.norm(g)
        if g_norm == 0.0:
            g_norm = 1e-8
        return (g / g_norm) * self.radius

    def prox_objective(self, x, g, L):
        """the objective the reference states, at a feasible x"""
        return L * self.phi(np.linalg.norm(x)) + np.dot(self.scaled(g), x)

    def prox_radius(self, L):
        return prox_radius(L, self.lamda, self.DS_mean, self.DS_mean_quad, self.radius)

    def prox_map(self, g, L):
        g_norm = np.linalg.norm(g)
        if g_norm == 0.0:
            g_norm = 1e-8
        return -(self.prox_radius(L) / g_norm) * g

    def div_prox_map(self, y, g, L):
        return self.prox_map(g - L * self.gradient(y), L)


def lmo_l2_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else center
        g_norm = np.linalg.norm(g)
        if g_norm < 1e-10:
            return c
        s = c - radius * g / g_norm
        assert abs(np.linalg.norm(s - c) - radius) <= 1e-10
        return s
    return f


def random_point_in_l2_ball(center, radius, spread_btm=0.1, spread_up=0.99, pos_dir=False):
    d = np.random.randn(len(center))
    d /= np.linalg.norm(d)
    if pos_dir:
        d = np.sign(d) * d
    rho = np.random.uniform(radius * spread_btm, radius * spread_up)
    return center + rho * d


def svm_label(row):
    """the label rule of generate_dataset_for_svm"""
    return 1 if (row > 0).sum() < row.size * 0.53 else -1


def ball_numbers(X, Y, lamda, center=None):
    """(radius, DS_mean, DS_mean_quad, L, x0) of svm_digits_ds_divs_ball"""
    n = X.shape[1]
    radius = min(n ** -1 * lamda ** -1 * np.sum(np.linalg.norm(X[:, :-1], axis=1)), (2 / lamda) ** 0.5)
    if center is None:
        center = np.zeros(n)
    h = PolyDiv(X, lamda=lamda, radius=radius)
    L = (h.DS_mean + min((2 * lamda) ** 0.5, h.DS_mean_quad)) * 0.08
    x0 = random_point_in_l2_ball(center, radius)
    return radius, h.DS_mean, h.DS_mean_quad, L, x0


# ---------------------------------------------------------------------------------------------- the stored runs
RUN_SEED = 2024
ITERS = 120


def run_table(mod, lmo_l2):
    """name -> call(f, poly_h, sq_h, L, x0, radius) -> (x, F, second trace) of the stored whole runs, on the solver
    functions of `mod` (the reference, the restatement above, or the package) -- the same table for all three"""
    N = ITERS
    return {
        "bpgls": lambda f, ph, sh, L, x0, R: mod.BPG(f, sh, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5)[:3],
        "abpg": lambda f, ph, sh, L, x0, R: mod.ABPG(f, sh, L, x0, gamma=2.0, maxitrs=N, theta_eq=False)[:3],
        "fwsq": lambda f, ph, sh, L, x0, R: mod.FW_alg_div_step(f, sh, L, x0, lmo=lmo_l2(R), maxitrs=N, gamma=2.0,
                                                               ls_ratio=2.0)[:3],
        "fwpoly": lambda f, ph, sh, L, x0, R: mod.FW_alg_div_step(f, ph, L, x0, lmo=lmo_l2(R), maxitrs=N, gamma=2.0,
                                                                 ls_ratio=2.0)[:3],
        "aibm_n0": lambda f, ph, sh, L, x0, R: mod.AIBM(f, sh, L, x0, gamma=2.0, maxitrs=N, noise=0)[:3],
        "aibm_n1": lambda f, ph, sh, L, x0, R: mod.AIBM(f, sh, L, x0, gamma=2.0, maxitrs=N, noise=0.1)[:3],
        "fgm": lambda f, ph, sh, L, x0, R: mod.AdaptFGM(f, sh, L, x0, maxitrs=N, noise=0.1)[:3],
    }


def driver_table(mod, lmo_l2, iters=40):
    """the solver calls of frank_wolfe_wtih_rs/ex_SVM.py:26-30 and aibm/ex_SVM.py:23-26 with poly_h"""
    N = iters
    return {
        "fw": lambda f, ph, L, x0, R: mod.FW_alg_div_step(f, ph, L, x0, lmo=lmo_l2(R), maxitrs=N, gamma=2.0,
                                                          ls_ratio=2.0)[:3],
        "bpgls": lambda f, ph, L, x0, R: mod.BPG(f, ph, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5)[:3],
        "abpg": lambda f, ph, L, x0, R: mod.ABPG(f, ph, L, x0, gamma=2.0, maxitrs=N, theta_eq=False)[:3],
        "aibm": lambda f, ph, L, x0, R: mod.AIBM(f, ph, L, x0, gamma=2.0, maxitrs=N, epsilon=1e-5, noise=0.1)[:3],
        "fgm": lambda f, ph, L, x0, R: mod.AdaptFGM(f, ph, L, x0, maxitrs=N, epsilon=1e-5, noise=0.1)[:3],
    }


class _Solvers:
    """the restatement's solver functions under the reference's names"""
    BPG = staticmethod(BPG)
    ABPG = staticmethod(ABPG)
    FW_alg_div_step = staticmethod(FW_alg_div_step)
    AIBM = staticmethod(AIBM)
    AdaptFGM = staticmethod(AdaptFGM)


SOLVERS = _Solvers
