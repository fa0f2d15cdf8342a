"""One Frank-Wolfe / Wolfe-Atwood step for D-optimal design, restated in plain NumPy from the prose of the reference
algorithm (accbpg/D_opt_alg.py:39-45, :59-61, :75-82, :145-147, :162-179) -- not from the kernels.

State: x (weights), H = (V diag(x) V^T)^-1 as maintained, w_k = v_k^T H v_k as tracked.  A step is a *probe* (which
column enters or leaves) followed by an *update* with five scalars (p, xscale, xadd, hcoef, hdiv):

    x  <- x * xscale;  x[p] += xadd
    Hv  = H v_p
    H  <- (H + hcoef * outer(Hv, Hv)) / hdiv
    w  <- (w + hcoef * (V^T Hv)^2) / hdiv

``update_f64`` is that in float64 with NumPy's own rounding (one rounding per written operation); ``update_ref`` is
the same in ``np.longdouble`` and also returns the magnitude sums that the forward bounds of the GPU tests are made of.

``axis_design`` builds inputs on which every sum of every kernel has at most one nonzero term (or only terms whose
partial sums are exact), so that float64 arithmetic in ANY order, partition or fused form gives the same bits."""
from collections import namedtuple
from fractions import Fraction

import numpy as np

Probe = namedtuple("Probe", "i j w_i w_j x_j")
Record = namedtuple("Record", "i j w_i w_j x_j q_prev logdet_H")     # what a solver's decision code reads

AWAY_THRESHOLD = 1.0e-8         # D_opt_alg.py:147


# ---------------------------------------------------------------------------------------------------------- probe
def probe(w, x, away):
    """(i, j, w_i, w_j, x_j).  i = np.argmax(w).  Frank-Wolfe: j is the first index of the minimum of w over the
    support x > 0 (:60-61, as an index into the full vector).  Away: j = np.argmin((w - w[i]) * (x > 1e-8)), formed
    exactly so (:146-147): one subtraction, one product with 1.0 or 0.0, first index of the minimum.  NumPy's NaN
    convention applies to both (the first NaN is the extremum)."""
    w = np.asarray(w, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    i = int(np.argmax(w))
    if away:
        with np.errstate(invalid="ignore"):
            d = (w - w[i]) * (x > AWAY_THRESHOLD)
        j = int(np.argmin(d))
    else:
        support = np.flatnonzero(x > 0)
        j = int(support[np.argmin(w[support])])
    return Probe(i, j, float(w[i]), float(w[j]), float(x[j]))


# --------------------------------------------------------------------------------------------------------- update
def update_x(x, p, xscale, xadd):
    """float64: x * xscale, then += xadd at p.  Two roundings per entry at most: the device's bits."""
    out = np.asarray(x, dtype=np.float64) * np.float64(xscale)
    out[p] += np.float64(xadd)
    return out


def setup_f64(V, x0):
    """(x, det(G), H, w) at the start (:39-45): G = V diag(x0) V^T, H = G^-1, w_k = v_k^T H v_k."""
    x = np.array(x0, dtype=np.float64)
    G = np.dot(V * x, V.T)
    H = np.linalg.inv(G)
    w = np.sum(V * np.dot(H, V), axis=0)
    return x, np.linalg.det(G), H, w


def update_f64(V, H, w, p, hcoef, hdiv):
    """(H', w') in float64, each written operation rounded once."""
    Hv = np.dot(H, V[:, p])
    Hn = (H + hcoef * np.outer(Hv, Hv)) / hdiv
    wn = (w + hcoef * np.dot(Hv, V) ** 2) / hdiv
    return Hn, wn


UpdateRef = namedtuple("UpdateRef", "Hv q H w u A Q B C")


def update_ref(V, H, w, p, hcoef, hdiv):
    """The update in np.longdouble from float64 inputs.  Returns Hv, q = v_p^T H v_p, H', w', u = V^T Hv and
        A_r = sum_c |H_rc| |v_c|              (|H| |v_p|: bounds Hv_r and its rounding error)
        Q   = sum_c |v_c| A_c                 (bounds q)
        B_k = sum_r A_r |V_rk|                (bounds u_k when Hv itself carries the error of A)
        C_k = sum_r |Hv_r| |V_rk|             (bounds u_k = V^T Hv for an exactly given Hv)"""
    L = np.longdouble
    Vl, Hl, wl = np.asarray(V, dtype=L), np.asarray(H, dtype=L), np.asarray(w, dtype=L)
    v = Vl[:, p]
    Hv = Hl.dot(v)
    q = v.dot(Hv)
    Hn = (Hl + L(hcoef) * np.outer(Hv, Hv)) / L(hdiv)
    u = Hv.dot(Vl)
    wn = (wl + L(hcoef) * u * u) / L(hdiv)
    A = np.abs(Hl).dot(np.abs(v))
    Q = np.abs(v).dot(A)
    B = A.dot(np.abs(Vl))
    Cs = np.abs(Hv).dot(np.abs(Vl))
    return UpdateRef(Hv, q, Hn, wn, u, A, Q, B, Cs)


def gamma(c):
    """c u / (1 - c u) with u = 2^-53: the relative error of c successive float64 roundings."""
    u = 2.0 ** -53
    return c * u / (1.0 - c * u)


# -------------------------------------------------------------------------------------------------- whole runs
def run_fw(V, x0, eps, maxitrs, decide):
    """D_opt_FW (:9-88) as a chain of probe / decide / float64 update.  ``decide(m, w_i, w_j, eps)`` is the solver's
    own scalar decision code (returns eps_pos, eps_neg, (xscale, xadd, hcoef, hdiv) or None, detmul).
    Returns (x, F, SP, SN, picks, (x, w, H)) with picks the list of (i, j)."""
    m = V.shape[0]
    x, det, H, w = setup_f64(V, x0)
    F, SP, SN, picks = [], [], [], []
    for _ in range(maxitrs):
        F.append(-np.log(det))
        pr = probe(w, x, 0)
        eps_pos, eps_neg, upd, detmul = decide(m, pr.w_i, pr.w_j, eps)
        SP.append(eps_pos); SN.append(eps_neg); picks.append((pr.i, pr.j))
        if upd is None:
            break
        x = update_x(x, pr.i, upd[0], upd[1])
        H, w = update_f64(V, H, w, pr.i, upd[2], upd[3])
        det *= detmul
    return x, np.array(F), np.array(SP), np.array(SN), picks, (x, w, H)


def run_away(V, x0, eps, maxitrs, make_run):
    """D_opt_FW_away (:91-185) likewise.  ``make_run(m, maxitrs)`` returns the solver's per-run decision object, whose
    ``iterate(k, record, collected, now, logdet_gram, eps)`` returns (p, xscale, xadd, hcoef, hdiv) or None and fills
    ``SP`` / ``SN``.  F[k] = log det(H_k) (:136)."""
    m = V.shape[0]
    x, det, H, w = setup_f64(V, x0)
    run = make_run(m, maxitrs)
    F, picks = [], []
    k = -1
    for k in range(maxitrs):
        F.append(np.log(np.linalg.det(H)))
        pr = probe(w, x, 1)
        picks.append((pr.i, pr.j))
        rec = Record(pr.i, pr.j, pr.w_i, pr.w_j, pr.x_j, float("nan"), float("nan"))
        upd = run.iterate(k, rec, float("nan"), 0.0, float(np.log(det)), eps)
        if upd is None:
            break
        x = update_x(x, upd[0], upd[1], upd[2])
        H, w = update_f64(V, H, w, upd[0], upd[3], upd[4])
    return x, np.array(F), run.SP[:k + 1].copy(), run.SN[:k + 1].copy(), picks, (x, w, H)


# -------------------------------------------------------------------------------------------------- axis designs
def axis_design(m, n, s, x0):
    """V with column k equal to s[k] * e_{k mod m}, and the diagonal G_rr = sum_k x0[k] s[k]^2 of V diag(x0) V^T
    (float64, summed in index order: exact under ``axis_exact``).  Returns (V, G)."""
    s = np.asarray(s, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    assert s.shape == (n,) and x0.shape == (n,)
    V = np.zeros((m, n))
    k = np.arange(n)
    V[k % m, k] = s
    G = np.zeros(m)
    np.add.at(G, k % m, x0 * s * s)
    return V, G


def _is_pow2(fr):
    return fr > 0 and (fr.numerator == 1 or fr.denominator == 1) and \
        (fr.numerator & (fr.numerator - 1)) == 0 and (fr.denominator & (fr.denominator - 1)) == 0


def axis_exact(m, s, x0):
    """The exactness preconditions of an axis design, in rational arithmetic.  Raises AssertionError naming the
    first that fails.
      1. every s_k^2 is a float64 (so w_k = s_k^2 / G_rr is one exact scaling by a power of two);
      2. every x_k s_k^2 is a float64, and within a row these terms are multiples of one power of two q with
         sum / q < 2^53: every partial sum of the Gram entry, in any order, with or without fma, is exact;
      3. every G_rr is an even power of two: sqrt, 1/sqrt, 1/G_rr are exact, and so are the Cholesky factor, its
         inverse W, H = W^T W = diag(1/G_rr), |W v_k|^2 and w_k;
      4. w_k = s_k^2 / G_rr neither overflows nor goes subnormal."""
    s = np.asarray(s, dtype=np.float64)
    x0 = np.asarray(x0, dtype=np.float64)
    n = len(s)
    # (the distinct (row, s, x0) triples and how often each occurs: a few, whatever n is)
    trip, count = np.unique(np.stack([np.arange(n) % m, s, x0], axis=1), axis=0, return_counts=True)
    rows = [[] for _ in range(m)]
    for (r, sk, xk), cnt in zip(trip, count):
        fs = Fraction(float(sk))
        sq = fs * fs
        assert Fraction(float(sk * sk)) == sq, "s^2 is not exact for s = %r" % sk
        if xk != 0.0:
            term = Fraction(float(xk)) * sq
            assert Fraction(float(xk * (sk * sk))) == term, "x0 s^2 is not exact for s = %r, x0 = %r" % (sk, xk)
            assert Fraction(float((sk * xk) * sk)) == term, "(s x0) s is not exact for s = %r, x0 = %r" % (sk, xk)
            rows[int(r)].append((term, int(cnt)))
    G = []
    for r in range(m):
        assert rows[r], "row %d has no supported column" % r
        total = sum(t * c for t, c in rows[r])
        q = Fraction(1, max(t.denominator for t, c in rows[r]))
        assert all((t / q).denominator == 1 for t, c in rows[r])
        assert total / q < 2 ** 53, "row %d: partial sums of the Gram entry are not exact" % r
        assert _is_pow2(total), "G[%d] = %s is not a power of two" % (r, total)
        e = total.numerator.bit_length() - total.denominator.bit_length()
        assert e % 2 == 0, "G[%d] = %s is not an EVEN power of two" % (r, total)
        G.append(total)
    for (r, sk, xk) in trip:
        wk = Fraction(float(sk)) ** 2 / G[int(r)]
        assert Fraction(2) ** -1020 < wk < Fraction(2) ** 1020, "w out of range for s = %r" % sk
        assert Fraction(float(wk)) == wk
    return [float(g) for g in G]


def axis_base(m, n, start, g_exp=None):
    """(s, x0) of the plain axis design the planted cases start from: s = 1 everywhere, x0 = 0 except on the 4m
    columns from ``start``, four per row, each with x0 = 2^(g_exp[r] - 2), so G_rr = 2^g_exp[r] (default 2^-4 in
    every row: w = 16 everywhere, a total tie).  Callers then change s on columns OUTSIDE the base, which leaves G
    alone."""
    assert 0 <= start and start + 4 * m <= n
    g_exp = np.full(m, -4) if g_exp is None else np.asarray(g_exp)
    s = np.ones(n)
    x0 = np.zeros(n)
    k = np.arange(start, start + 4 * m)
    x0[k] = np.ldexp(1.0, g_exp[k % m] - 2)
    return s, x0


RUN_SHAPES = [(8, 40, 0), (16, 4608, 1024), (16, 131072 + 257, 1024)]      # (m, n, first base column)


def axis_run_design(m, n, start):
    """(s, x0) of the axis designs the whole-run tests use.  Rows differ in G_rr (2^-2, 2^-4, 2^-6; for m = 16 the
    weights sum to one), the base columns have s = 1, and outside the base s = 2 on two fifths of the last quarter
    of the columns (so the maxima of w tie exactly within a row and sit at high indices) and s = 1/2 on a few early
    columns.  With 60 iterations the away variant takes Frank-Wolfe steps, then away steps (checked by
    test_fw_step_cpu.test_run_designs_take_both_kinds_of_step), and every tracked w on the support stays above 1, where
    the reference's step-length formula is meaningful."""
    assert m in (8, 16)
    g_exp = np.array([-2] * 2 + [-4] * 6 + [-6] * 8) if m == 16 else np.array([-2] * 3 + [-4] * 3 + [-6] * 2)
    s, x0 = axis_base(m, n, start, g_exp)
    k = np.arange(n)
    outside = (k < start) | (k >= start + 4 * m)
    s[outside & (k >= n - n // 4) & ((k * 7 % 5) < 2)] = 2.0
    s[outside & (k < n // 2) & (k % 11 == 3)] = 0.5
    return s, x0
