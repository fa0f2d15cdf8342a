"""NumPy side of the (L0, L1) Frank-Wolfe tests: the instance, a stand-in objective, the oracles, a driver for the run
objects of accbpg_and_fw_amd/solver_runs.py, the table of stored runs and the carried-margin bound.  Shared by
tests/test_l0l1_cpu.py, tests/test_gpu_l0l1.py and tools/gen_golden_l0l1.py.  The package does not import this module.

The instance is ill-conditioned on purpose: Gaussian rows with Toeplitz covariance rho^|i-j|, rho = 0.95, through its
Cholesky factor, columns scaled by 10^linspace(0, 1, n), labels from a planted vector with a little noise.

The stand-in objective is written with library routines (np.logaddexp, scipy.special.expit), not with the formulas of
the device's epilogue, so the goldens do not depend on tests/logistic_numpy.py; `perturb` multiplies the margins by
1 + 4e-16*N(0,1), the stand-in for another summation order (tools/gen_golden_logistic.py).

`drive` runs a run object with NumPy vectors in the reference's own expressions -- np.linalg.norm, np.dot / np.vdot,
x + alpha*d -- so that with the same objective it reproduces the reference bit for bit.

Carried margins.  With carry=True the margin of row i after an accepted step is fma(a, (A d)_i, z_i) in the place of
(A (x + a d))_i; tests/test_gpu_logistic_line.py derives |ds_i| <= gamma(device_chain(n) + 2)(|A||x| + |a||A||d|)_i per
step.  The iterates stay in the domain, |x|_1 <= X1 and |d|_1 <= 2*X1 with a <= 1, so one step moves a value by at most
    value_step_bound = gamma(device_chain(n) + 2) * 3 * X1 * max_ij |A_ij|
and k carried steps by k times that; X1 is the domain's largest l1 norm (sqrt(n) R, n R, R)."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import logistic_numpy as LN  # noqa: E402

SHAPE = (120, 60)
SEED = 11
RHO = 0.95
COL_SCALE = 10.0
ITERS = 60
REFRESH = 64


def toeplitz(n, rho):
    idx = np.arange(n)
    return rho ** np.abs(idx[:, None] - idx[None, :])


def instance(seed=SEED, shape=SHAPE):
    """(A, y) of the stored runs"""
    m, n = shape
    rng = np.random.RandomState(seed)
    chol = np.linalg.cholesky(toeplitz(n, RHO))
    A = rng.randn(m, n).dot(chol.T) * (COL_SCALE ** np.linspace(0, 1, n))[None, :]
    w = rng.randn(n)
    w /= np.linalg.norm(w)
    y = np.sign(0.5 * A.dot(w) + 0.01 * rng.randn(m))
    y[y == 0] = 1.0
    return A, y


class StandIn:
    """logistic regression under the reference's func_grad protocol"""

    def __init__(self, X, y, perturb=None):
        self.X, self.y = X, np.asarray(y, dtype=np.float64).reshape(-1)
        self.m, self.n = X.shape
        self._rng = perturb
        self.values = 0                                         # value-only calls: the trials of a run

    def func_grad(self, x, flag=2):
        from scipy.special import expit
        z = np.dot(self.X, x)
        if self._rng is not None:
            z = z * (1 + 4e-16 * self._rng.randn(z.size))
        s = self.y * z
        f = np.sum(np.logaddexp(0.0, -s)) / self.m
        if flag == 0:
            self.values += 1
            return f
        g = np.dot(-(self.y * expit(-s)), self.X) / self.m
        return g if flag == 1 else (f, g)

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)


class SquaredL2Norm:
    def extra_Psi(self, x):
        return 0

    def divergence(self, x, y):
        xy = x - y
        return 0.5 * np.dot(xy, xy)


def lmo_l2_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else center
        g_norm = np.linalg.norm(g)
        return np.array(c) if g_norm < 1e-10 else c - radius * g / g_norm
    return f


def lmo_linf_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else center
        return c - radius * np.sign(g)
    return f


def lmo_simplex(radius=1):
    def f(g):
        s = np.full(g.shape, 1e-15)
        s[np.argmin(g)] = radius
        return s
    return f


def drive(run, f, h, x0, maxitrs, lmo, want_div, tests=None):
    """One solve by a run object of solver_runs.py on NumPy vectors -> run.result(x).  tests: a list that receives
    (lhs, rhs) of every acceptance test."""
    x = np.copy(x0)
    for k in range(maxitrs):
        fx, g = f.func_grad(x)
        run.begin(k, fx, fx + h.extra_Psi(x), 0.0)
        s = lmo(g)
        d = s - x
        slope = np.dot(g.ravel(), d.ravel()) if want_div else np.vdot(g, d)
        if not run.direction(np.linalg.norm(g), slope, h.divergence(s, x) if want_div else np.linalg.norm(d)):
            break
        while True:
            a = run.step()
            x1 = x + a * d
            if not run.linesearch:
                break
            ok = run.accepts(f.func_grad(x1, flag=0))
            if tests is not None:
                tests.append((run.lhs, run.rhs))
            if ok:
                break
        x = x1
        if run.finish():
            break
    return run.result(x)


# ------------------------------------------------------------------------------------------------- the stored runs
RADIUS = {"l2": 1.0, "linf": 0.05, "simplex": 1.0}
SOLVERS = ("shortest", "loglin", "logonly")
DOMAINS = ("l2", "linf", "simplex")


def start(domain, n):
    return np.full(n, 1.0 / n) if domain == "simplex" else np.zeros(n)


def l1_reach(domain, n):
    """the largest l1 norm of a point of the domain"""
    R = RADIUS[domain]
    return {"l2": np.sqrt(n) * R, "linf": n * R, "simplex": R + n * 1e-15}[domain]


def constants(A):
    """(L0, L1) the runs start from: L1 from the largest row norm, as the reference's generators take it"""
    return 1e-3, float(np.max(np.linalg.norm(A, axis=1)))


def run_params(solver, domain, A):
    """keyword arguments of the stored run, the reference's names"""
    L0, L1 = constants(A)
    if solver == "shortest":
        return dict(L0=L0, L1=L1, gamma=2.0, ls_ratio=2)
    p = dict(L0=L0, L1=L1, ls_ratio=2.0)
    if domain == "l2":
        p["L1_max"] = L1 / 4                                    # a cap that binds
    return p


def call_solver(mod, solver, f, h, x0, lmo, params, **extra):
    """the solver `solver` of `mod` (the reference or the package) -> (x, F, Ls, LOG_STEPS or None)"""
    p = dict(params)
    if solver == "shortest":
        out = mod.FW_alg_L0_L1_shortest_step(f, h, p.pop("L0"), p.pop("L1"), x0, ITERS, lmo=lmo, verbose=False, **p,
                                             **extra)
        return out[0], out[1], out[2], None
    fn = mod.FW_l0l1_log_and_linear_step if solver == "loglin" else mod.FW_l0l1_log_only
    out = fn(f, h, p.pop("L0"), p.pop("L1"), x0, ITERS, lmo, p.pop("ls_ratio"), verbose=False, **p, **extra)
    return out[0], out[1], out[2], out[3]


def make_run(R, solver, params):
    """the run object of solver_runs (module R) for the stored run's parameters"""
    p = dict(params)
    if solver == "shortest":
        return R._ShortestStepRun(p["L0"], p["L1"], p["gamma"], 1e-14, True, p["ls_ratio"])
    cls = R._LogLinearRun if solver == "loglin" else R._LogOnlyRun
    return cls(p["L0"], p["L1"], p["ls_ratio"], 1e-14, p.get("L0_max"), p.get("L1_max"), True)


def value_step_bound(A, domain):
    n = A.shape[1]
    return LN.gamma(LN.device_chain(n) + 2) * 3 * l1_reach(domain, n) * float(np.max(np.abs(A)))
