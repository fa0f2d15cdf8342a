"""Restatement, references, exact data and forward bounds for the logistic family: LogisticRegression
(logistic_kernels.hip) and L2L1Linf (vec_kernels.hip), shared by tests/test_logistic_cpu.py, the GPU modules
tests/test_gpu_logistic.py, test_gpu_guard_logistic.py and test_gpu_stream_logistic.py, and
tools/gen_golden_logistic.py.
The package does not import this module.

The restatement.  LogisticRegression below is the objective of accbpg/ex_LR_L2L1Linf.py:19-54 in the operation order of
the device's per-row epilogue, in float64 NumPy, one rounding per operation:

    s = y_i*z            a = |s|            e = exp(-a)
    t_i = max(-s, 0) + log1p(e)                         log(1 + exp(-s)): nothing overflows, nothing cancels
    q   = (s >= 0) ? e/(1 + e) : 1/(1 + e)              sigma(-s)
    r_i = -(y_i*q)                                      grad f = A^T r / m,   f = sum_i t_i / m

L2L1Linf is accbpg/functions.py:782-835 restated elementwise (IEEE arithmetic: it must have the reference's bits).

Exact data.  exact_data(m, n, seed) draws A with integers in [-4, 4], x with multiples of 1/64 in [-4, 4], y = +-1:
A x is a sum of at most 2^15 integers below 2^10 in units of 1/64, exact in float64 in any order, and so is s = y*z.
planted(m, n, seed) sets x_0 = 1 and turns the first rows into k*e_0, so that s takes each value of PLANTED_S exactly
(+-inf through y = +-inf with k = 1, NaN through y = NaN).

Allowances.  T_ULP and Q_ULP are the allowances, in ulps of the result, for the float64 evaluation of t and q from an
exact s by any math library.  They are measured, not derived: NumPy's float64 formulas against the np.longdouble
evaluation (64-bit significand; cross-checked against mpmath at 40 digits on the planted values) over the margins of
exact data and the planted values gave at most T_MEASURED ulp for t and Q_MEASURED ulp for q; each is rounded up to a
whole ulp, plus one ulp for a different math library (the rule of tests/poisson_numpy.py for LOG).
test_logistic_cpu.py repeats the measurement.

Forward bounds, u = 2^-53, gamma_k = k*u/(1 - k*u).  One ulp of a normal v is at most 2u*|v|; below the normal range
an ulp is 2^-1074 whatever v is (exp(-745) is a single subnormal step), so an allowance of K ulps of v is
ulps(K, v) = K*max(2u*|v|, 2^-1074).

  rows, exact data      |t^_i - t_i| <= ulps(T, t_i),    |r^_i - r_i| <= ulps(Q, r_i)        (y = +-1: y*q is exact)
  value.  The t^_i are added on the fixed tree of csrc/reduce.hpp with the block cap of vec_kernels.hip: a term passes
  the trips of its thread, six shuffle levels and three wave additions of the block stage, then the record additions
  and the block stage of the final launch -- D = reduce_numpy.tree_depth(m, 1024) additions, each rounded once:
      |sum^ - sum_i t_i| <= sum_i ulps(T, t_i) + gamma_D * sum_i t_i,         f = sum^/m adds u*f
  gradient.  A column's sum is a chain of fma(r_i, A_ij, acc), one rounding each, over the at most ceil(m/nsplit) rows
  of a split, then a sequential sum of nsplit <= 64 partials -- at most m + 64 roundings -- and one division by m;
  with one more u to spare for second-order terms
      |g^_j - g_j| <= (Q*2u + u + gamma_(m+64)) * sum_i |A_ij||r_i| / m + u*|g_j|

  general data.  On the device a product A_ij x_j passes at most C = ceil(n/64) + 12 roundings on its way into z^_i: a
  lane's chain of fma (at most ceil(n/64) with scalar loads and a wavefront per row, fewer in every other form), the
  one-column tail fma, s0 + s1, six shuffle levels, and the four wave additions of the workgroup form.  A float64
  NumPy dot product (the goldens) may pass n.  s = y*z is rounded once:
      |ds_i| <= gamma_C * |y_i| * sum_j |A_ij x_j| + u*|s_i|            (C = n for the NumPy values)
  softplus is 1-Lipschitz and sigma is 1/4-Lipschitz, and y*q is rounded once when y is not +-1:
      |t^_i - t_i| <= ulps(T, t_i) + |ds_i|,        |r^_i - r_i| <= ulps(Q, r_i) + |y_i|*|ds_i|/4 + u*|r_i|
  and the sums take these in the place of ulps(T, t_i) and Q*2u*|r_i|.

The np.longdouble reference sums m terms with an error below m*2^-64 of the same sums of magnitudes, 2^-11 of the
gamma terms."""
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(_HERE))
sys.path.insert(0, _HERE)
import reduce_numpy as T  # noqa: E402
from oracle.np_oracle import ABDA, ABPG, ABPG_expo, ABPG_gain, BPG, FW_alg_div_step  # noqa: E402,F401
from inexact_numpy import SquaredL2Norm  # noqa: E402,F401
from poisson_numpy import ax_form, vt_nsplit  # noqa: E402,F401

U = 2.0 ** -53
TINY = 2.0 ** -1074
LD = np.longdouble
T_MEASURED = 1.39             # NumPy fp64 t against np.longdouble, in ulps (20 000 exact-data margins and PLANTED_S)
Q_MEASURED = 1.84             # the same for q
T_ULP = 3                     # ceil(T_MEASURED) + 1
Q_ULP = 3                     # ceil(Q_MEASURED) + 1

PLANTED_S = [0.0, -0.0, 36.0, -36.0, 37.0, -37.0, 50.0, -50.0, 700.0, -700.0, 745.0, -745.0, 746.0, -746.0, 1e4, -1e4,
             np.inf, -np.inf, np.nan]

GOLDEN = os.path.join(_HERE, "golden")
GAUSS = dict(m=96, n=40, seed=17)                 # the per-call instance of the goldens: rebuilt, never stored
EXAMPLE = dict(m=100, n=200, seed=2025, B=1.0)    # the whole-run instance: the shape of ex_LR_L2L1Linf.py:59-60
ITERS = 100
KERNEL_L = (0.05, 40.0)
EXACT_SHAPES = [(1, 1), (3, 2), (4, 64), (5, 65), (7, 129), (33, 4096), (5, 4097), (2050, 130), (416, 1540)]
LONG_SHAPE = (2048, 32768)
PLANTED_SHAPES = [(7, 129), (33, 4096)]


def gamma(k):
    return k * U / (1 - k * U)


def ulps(k, v):
    """an allowance of k ulps of v (float64), as a bound on an absolute error"""
    return k * np.maximum(2 * U * np.abs(v), TINY)


# ------------------------------------------------------------------------------------------------------- the data
def gaussian_instance(m=GAUSS["m"], n=GAUSS["n"], seed=GAUSS["seed"]):
    """(A, y): N(0,1) features, labels +-1 from a noisy random hyperplane"""
    rng = np.random.RandomState(seed)
    A = rng.randn(m, n)
    w = rng.randn(n)
    y = np.where(A.dot(w) + 0.5 * rng.randn(m) > 0, 1.0, -1.0)
    return A, y


def box_points(n, B=1.0):
    """three points of the box ||x||_inf <= B"""
    rng = np.random.RandomState(23)
    return np.array([rng.uniform(-B, B, n) * s for s in (0.1, 0.5, 1.0)])


def example_draws(m=EXAMPLE["m"], n=EXAMPLE["n"], seed=EXAMPLE["seed"]):
    """(A, b) as ex_LR_L2L1Linf.py:61-63 draws them from the legacy generator under `seed`; b is all +1"""
    np.random.seed(seed)
    A = np.random.randn(m, n)
    b = np.sign(np.random.rand(m, 1))
    return A, b


def example_labels(m=EXAMPLE["m"]):
    """mixed +-1 labels for the whole runs, from a generator of their own"""
    return np.random.RandomState(91).choice([-1.0, 1.0], size=m)


def exact_data(m, n, seed):
    rng = np.random.RandomState(seed)
    A = rng.randint(-4, 5, size=(m, n)).astype(np.float64)
    x = rng.randint(-256, 257, size=n) / 64.0
    y = rng.choice([-1.0, 1.0], size=m)
    return A, x, y


PLANTED_SHORT = [0.0, -0.0, 746.0, -746.0, np.inf, -np.inf, np.nan]      # the seven that a 7-row matrix holds


def planted(m, n, seed, values=None):
    """exact data whose first rows have s = values[k] exactly (default: PLANTED_S, or PLANTED_SHORT when m is too small
    for it); returns (A, x, y, s).  A row with y = +inf has q = 0 and r = -(inf*0) = NaN, one with y = -inf has q = 1
    and r = +inf."""
    A, x, y = exact_data(m, n, seed)
    x[0] = 1.0
    if values is None:
        values = PLANTED_S if m >= len(PLANTED_S) else PLANTED_SHORT
    k = len(values)
    assert k <= m
    for i, s in enumerate(values):
        A[i] = 0.0
        if np.isfinite(s):
            A[i, 0], y[i] = abs(s), (-1.0 if np.signbit(s) else 1.0)
        else:
            A[i, 0], y[i] = 1.0, s
    return A, x, y, np.array(values)


# ------------------------------------------------------------------------------------------------ the restatement
def epilogue(z, y):
    """(t, r) of the rows from z = A x in float64, the device's operation order"""
    with np.errstate(all="ignore"):
        s = y * z
        a = np.abs(s)
        e = np.exp(-a)
        ns = -s
        hi = np.where(ns > 0.0, ns, 0.0)
        t = hi + np.log1p(e)
        den = 1.0 + e
        q = np.where(s >= 0.0, e / den, 1.0 / den)
        r = -(y * q)
    return t, r


def tq_fp64(s):
    """(t, q) of float64 margins s by the same formulas"""
    t, r = epilogue(np.asarray(s, dtype=np.float64), np.float64(1.0))
    return t, -r


def tq_ref(s):
    """np.longdouble (t, q) of float64 margins s"""
    with np.errstate(all="ignore"):
        s = np.asarray(s, dtype=LD)
        e = np.exp(-np.abs(s))
        t = np.maximum(-s, LD(0)) + np.log1p(e)
        q = np.where(s >= 0, e / (1 + e), 1 / (1 + e))
    return t, q


def tq_mp(s):
    """(t, q) of one finite float64 margin at 40 digits (mpmath), as np.longdouble"""
    import mpmath
    with mpmath.workdps(40):
        sm = mpmath.mpf(float(s))
        t = mpmath.log1p(mpmath.exp(-sm)) if sm >= 0 else -sm + mpmath.log1p(mpmath.exp(sm))
        q = 1 / (1 + mpmath.exp(sm))
        return LD(mpmath.nstr(t, 30)), LD(mpmath.nstr(q, 30))


def ulp_error(got, ref):
    """|got - ref| in ulps of the float64 result, entry by entry (finite entries)"""
    got = np.asarray(got, dtype=np.float64)
    return np.abs(LD(got) - ref) / LD(np.spacing(np.abs(got)))


def measure_tq(margins):
    """the largest error of NumPy's fp64 t and q against np.longdouble over finite margins, in ulps"""
    s = np.asarray(margins, dtype=np.float64)
    s = s[np.isfinite(s)]
    t, q = tq_fp64(s)
    tr, qr = tq_ref(s)
    return float(np.max(ulp_error(t, tr))), float(np.max(ulp_error(q, qr)))


def measured_margins(count=20000):
    """margins of exact data at the small shapes of the GPU module, and the planted values"""
    out, seed = [np.array(PLANTED_S)], 0
    while sum(v.size for v in out) < count:
        for m, n in EXACT_SHAPES[:5] + [(2050, 130)]:
            A, x, y = exact_data(m, n, 1000 + seed)
            out.append(y * A.dot(x))
            seed += 1
    return np.concatenate(out)


class LogisticRegression:
    """the restatement; `perturb` (a RandomState) multiplies the margins by 1 + 4e-16*N(0,1), the stand-in for another
    summation order that tools/gen_golden_logistic.py uses"""

    def __init__(self, X, y, alpha=0.01, perturb=None):
        self.X, self.y, self.alpha = X, np.asarray(y, dtype=np.float64).reshape(-1), alpha
        self.m, self.n = X.shape
        self._rng = perturb

    def _z(self, x):
        z = np.dot(self.X, x)
        if self._rng is not None:
            z = z * (1 + 4e-16 * self._rng.randn(z.size))
        return z

    def f(self, x):
        return self.func_grad(x, 0)

    def __call__(self, x):
        return self.func_grad(x, 0)

    def gradient(self, x):
        return self.func_grad(x, 1)

    def func_grad(self, x, flag=2):
        t, r = epilogue(self._z(x), self.y)
        if flag == 0:
            return np.sum(t) / self.m
        g = np.dot(r, self.X) / self.m
        if flag == 1:
            return g
        return np.sum(t) / self.m, g


def clip_keep_nan(v, B):
    v = np.where(v < -B, -B, v)
    return np.where(v > B, B, v)


class L2L1Linf:
    def __init__(self, lamda=0, B=1):
        self.lamda, self.B = lamda, B

    def __call__(self, x):
        return 0.5 * np.dot(x, x)

    def extra_Psi(self, x):
        return self.lamda * np.sum(np.abs(x))

    def gradient(self, x):
        return x

    def divergence(self, x, y):
        assert x.shape == y.shape
        xy = x - y
        return 0.5 * np.dot(xy, xy)

    def prox_terms(self, y, g, L):
        """(v, thr) before the threshold: v = -((1/L)*(g - L*y))"""
        w = g if y is None else g - L * y
        return -((1.0 / L) * w), self.lamda / L

    def prox_map(self, g, L, y=None):
        assert L > 0
        with np.errstate(invalid="ignore"):
            v, thr = self.prox_terms(y, g, L)
            v = np.where(np.abs(v) <= thr, 0.0, v)
            v = np.where(v > thr, v - thr, v)
            v = np.where(v < -thr, v + thr, v)
            return clip_keep_nan(v, self.B)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape and L > 0
        return self.prox_map(g, L, y=y)

    def ls_elementwise(self, g, x, y, z=None, z1=None):
        """the per-entry terms of (<g,x-y>, sum (x-y)^2, sum (z-z1)^2); a term that is not wanted is None"""
        d = x - y
        dz = None if z is None else z - z1
        return (None if g is None else g * d), d * d, (None if dz is None else dz * dz)


def lmo_linf_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else np.array(center)
        return c - radius * np.sign(g)
    return f


# ---------------------------------------------------------------------------------------------------- the bounds
def device_chain(n):
    """the most roundings a product passes on its way into a row sum of pass 1, in any launch form"""
    return -(-n // 64) + 12


def ds_bound(A, x, y, s, chain=None):
    """|ds_i| of general data; chain: the roundings of a row sum (default: the device's, n for a NumPy dot product)"""
    k = device_chain(A.shape[1]) if chain is None else chain
    return gamma(k) * np.abs(y) * np.abs(A).dot(np.abs(x)) + U * np.abs(s)


def row_refs(z, y):
    """np.longdouble (t, r) of the rows from float64 z = A x and labels y"""
    s = np.asarray(y, dtype=LD) * np.asarray(z, dtype=LD)
    t, q = tq_ref(s)
    return t, -(np.asarray(y, dtype=LD) * q)


def refs_and_bounds(A, z, y, ds=None):
    """From the float64 z = A x the rows were computed from (exact on exact data): np.longdouble references and bounds
    -> dict(t, r, t_bound, r_bound, f, f_bound, g, g_bound).  ds: the |ds_i| of general data, None on exact data."""
    m = A.shape[0]
    t, r = row_refs(z, y)
    tb, rb = ulps(T_ULP, t), ulps(Q_ULP, r)
    if ds is not None:
        tb = tb + ds
        rb = rb + np.abs(y) * ds / 4 + U * np.abs(r)
    depth = T.tree_depth(m, T.CAP_VEC)
    f = np.sum(t) / m
    fb = (np.sum(tb) + gamma(depth) * np.sum(np.abs(t))) / m + U * np.abs(f)
    Al = np.abs(np.asarray(A, dtype=LD))
    g = r.dot(np.asarray(A, dtype=LD)) / m
    gb = (rb.dot(Al) + (U + gamma(m + 64)) * np.abs(r).dot(Al)) / m + U * np.abs(g)
    return dict(t=t, r=r, t_bound=tb, r_bound=rb, f=f, f_bound=fb, g=g, g_bound=gb)


def all_shapes():
    """every (m, n) the GPU module evaluates on exact data"""
    return EXACT_SHAPES + [LONG_SHAPE]


# ---------------------------------------------------------------------------------------------- the stored runs
def run_table(mod, lmo_linf):
    """name -> call(f, h, sq_h, L, x0, B) -> (x, F, second trace) of the stored whole runs, on the solver functions of
    `mod` (the reference, the restatement's, or the package) -- the same table for all three"""
    N = ITERS

    def gain(f, h, sh, L, x0, B):                   # ex_LR_L2L1Linf.py:75-76
        out = mod.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, restart=False)
        return out[0], out[1], out[3]

    def expo(f, h, sh, L, x0, B):
        out = mod.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=N)
        return out[0], out[1], out[3]

    return {
        "bpg": lambda f, h, sh, L, x0, B: mod.BPG(f, h, L, x0, maxitrs=N, linesearch=False)[:3],
        "bpgls": lambda f, h, sh, L, x0, B: mod.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5)[:3],
        "abpg": lambda f, h, sh, L, x0, B: mod.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=False)[:3],
        "gain": gain,
        "expo": expo,
        "abda": lambda f, h, sh, L, x0, B: mod.ABDA(f, h, L, x0, gamma=2.0, maxitrs=N)[:3],
        "fw": lambda f, h, sh, L, x0, B: mod.FW_alg_div_step(f, sh, L, x0, lmo=lmo_linf(B), maxitrs=N, gamma=2.0,
                                                             ls_ratio=2.0)[:3],
    }


class _Solvers:
    """the restatement's solver functions under the reference's names"""
    BPG = staticmethod(BPG)
    ABPG = staticmethod(ABPG)
    ABPG_gain = staticmethod(ABPG_gain)
    ABPG_expo = staticmethod(ABPG_expo)
    ABDA = staticmethod(ABDA)
    FW_alg_div_step = staticmethod(FW_alg_div_step)


SOLVERS = _Solvers
