"""NumPy restatement of D_opt_FW_div_step / D_opt_FW_descent_step (accbpg_and_fw_amd/D_opt_alg.py) and of one record
of accbpg_fw_div_probe_step, written from DESIGN.md 6f: float64 state (x, H = (V X V^T)^-1, w = diag(V^T H V))
maintained by rank-one updates, the host arithmetic in plain Python floats in the order the solver writes it.
Imports nothing from the package; the GPU and the CPU tests compare against it."""
import math

import numpy as np

FILL = 1e-15
FLOOR = 1e-6


class State:
    """x, H, w and the scalars beside them: ld = log det of the tracked Gram matrix, q = floor mass not in it."""

    def __init__(self, V, x0):
        self.V = np.ascontiguousarray(V, dtype=np.float64)
        self.m, self.n = self.V.shape
        self.init(np.array(x0, dtype=np.float64))

    def init(self, x):
        self.x = x.copy()
        G = (self.V * self.x) @ self.V.T
        try:
            Lc = np.linalg.cholesky(G)
        except np.linalg.LinAlgError:
            raise ValueError("HXHT is singular or not positive definite")
        self.ld = 2.0 * float(np.sum(np.log(np.diag(Lc))))
        W = np.linalg.solve(Lc, np.eye(self.m))
        self.H = W.T @ W
        self.w = np.sum((W @ self.V) ** 2, axis=0)
        self.q = 0.0
        self.since = 0

    def probe(self, value, fill=FILL):
        return probe_record(self.V, self.H, self.w, self.x, fill, value)

    def apply(self, rec, a, value, hcoef, hdiv, fill=FILL):
        s = np.full(self.n, fill)
        s[rec["i"]] = value
        d = s - self.x
        self.x = self.x + a * d
        hv = rec["hv"]
        self.H = (self.H + hcoef * np.outer(hv, hv)) / hdiv
        self.w = (self.w + hcoef * rec["u"] ** 2) / hdiv


def probe_record(V, H, w, x, fill, value):
    """The fields of accbpg_fw_div_probe (NumPy summation order) plus hv and u of the direction."""
    i = int(np.argmin(-w))
    s = np.full(x.shape, fill)
    s[i] = value
    with np.errstate(all="ignore"):
        r = s / x
        div = float(np.sum(r - np.log(r) - 1.0))
        slope = float(np.sum((-w) * (s - x)))
    hv = H @ V[:, i]
    u = hv @ V
    return dict(i=i, w_i=float(w[i]), x_i=float(x[i]), sum_w=float(np.sum(w)), sum_w2=float(np.sum(w * w)),
                slope=slope, div=div, min_x=float(np.min(x)), sum_u2=float(np.sum(u * u)), hv=hv, u=u)


def step_scalars(a, radius, rec, ld, q, m, fill=FILL):
    """(hcoef, hdiv, ld1, q1, f1) of a step of length a < 1 towards the vertex of `rec`."""
    tau = a * (radius - fill) / (1 - a)
    den = 1 + tau * rec["w_i"]
    hcoef = -tau / den
    hdiv = 1 - a
    ld1 = ld + m * math.log(hdiv) + math.log(den)
    q1 = q + a * (fill - q)
    sw1 = (rec["sum_w"] + hcoef * rec["sum_u2"]) / hdiv
    f1 = -ld1 - q1 * sw1
    return hcoef, hdiv, ld1, q1, f1


def _value(V, x):
    G = (V * x) @ V.T
    try:
        Lc = np.linalg.cholesky(G)
    except np.linalg.LinAlgError:
        raise ValueError("HXHT is singular or not positive definite")
    return -2.0 * float(np.sum(np.log(np.diag(Lc))))


def fw_div_step(V, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1, refresh=256):
    """-> (x, F, Ls)"""
    if ls_ratio < 1:
        raise ValueError("ls_ratio must be >= 1")
    if L <= 0:
        raise ValueError("Initial L must be positive")
    if epsilon <= 0:
        raise ValueError("epsilon must be positive")
    st = State(V, x0)
    m = st.m
    F = np.zeros(maxitrs)
    Ls = np.zeros(maxitrs)
    done = 0
    for k in range(maxitrs):
        if refresh and st.since == refresh:
            st.init(st.x)
        rec = st.probe(radius)
        fx = -st.ld - st.q * rec["sum_w"]
        F[k] = fx
        div = rec["div"] if rec["div"] != 0 else FLOOR
        slope = rec["slope"]
        if 0 < slope <= FLOOR:
            slope = 0.0
        if slope > 0:
            raise ValueError("grad_d_prod must be non-positive")
        assert rec["min_x"] > 0, "Entries of x or y not positive."
        if linesearch:
            L = L / ls_ratio
        while True:
            a = min((-slope / (2 * L * div)) ** (1 / (gamma - 1)), 1.0)
            if a < 1:
                hcoef, hdiv, ld1, q1, f1 = step_scalars(a, radius, rec, st.ld, st.q, m)
                trial = None
            else:
                s = np.full(st.n, FILL)
                s[rec["i"]] = radius
                trial = st.x + a * (s - st.x)
                f1 = _value(st.V, trial) if linesearch else None
            if not linesearch:
                break
            assert not math.isinf(L), "L is infinite"
            if f1 <= fx + a * slope + a ** gamma * L * div:
                break
            L = L * ls_ratio
        if trial is None:
            st.apply(rec, a, radius, hcoef, hdiv)
            st.ld, st.q = ld1, q1
            st.since += 1
        else:
            st.init(trial)
        Ls[k] = L
        done = k + 1
        if k > 0 and abs(F[k] - F[k - 1]) < epsilon:
            break
    return st.x, F[:done], Ls[:done]


def fw_descent_step(V, x0, maxitrs, epsilon=1e-14, radius=1, refresh=256):
    """-> (x, F)"""
    st = State(V, x0)
    m = st.m
    F = np.zeros(maxitrs)
    rec = st.probe(radius)
    F[0] = -st.ld - st.q * rec["sum_w"]
    k = 0
    for k in range(1, maxitrs):
        a = 2 / (k + 2)
        hcoef, hdiv, ld1, q1, _ = step_scalars(a, radius, rec, st.ld, st.q, m)
        st.apply(rec, a, radius, hcoef, hdiv)
        st.ld, st.q = ld1, q1
        st.since += 1
        if refresh and st.since == refresh:
            st.init(st.x)
        rec = st.probe(radius)
        F[k] = -st.ld - st.q * rec["sum_w"]
        if abs(F[k] - F[k - 1]) < epsilon or math.sqrt(rec["sum_w2"]) < epsilon:
            break
    return st.x, F[:k + 1]
