"""Exact data, references and forward bounds for the two row passes of poisson_kernels.hip (PoissonRegression and
KLdivRegression), shared by tests/test_poisson_forms_cpu.py and tests/test_gpu_poisson_forms.py.

Exact data.  exact_poisson(m, n, seed) draws A with integers in [1, 8], x with multiples of 1/64 in [1/64, 4] and a
row factor p_i from {1/4, 1/2, 3/4, 1, 5/4, 3/2, 2}, and sets b = (A x) * p.  A x is a sum of at most 2^15 integers
below 2^11, in units of 1/64: every product and every sum is exact in float64 in any order, so is b (p has three
bits), and b/Ax is exactly p because IEEE division is correctly rounded and the quotient is representable.
r = 1 - p is a multiple of 1/4, so g = A^T r is exact in any order and under any row split, and a row with p = 1 has
t_i = b*log(1) + Ax - b = 0 exactly.  exact_kl(m, n, seed) is the same with p from {1/4, 1/2, 1, 2, 4}: Ax/b = 1/p
exactly, and r = log(1/p) is the only inexact step of the KL pass.

What is compared bit for bit: fitted() (A x) of both objectives, the Poisson gradient, and f = 0, g = 0 where every
p_i = 1.  What gets a forward bound, against an np.longdouble evaluation of the reference's formulas
(accbpg/functions.py:104-120 and 142-158), with u = 2^-53, gamma_k = k*u/(1 - k*u), ell_i = |log(b_i/Ax_i)|:

  Poisson f.  A row computes lg = log(q)(1 + d0), p = b*lg (1 + d1), s = (p + Ax)(1 + d2), t = (s - b)(1 + d3) with
  |d0| <= LOG*2u (LOG ulps of the logarithm, one ulp being at most 2u of the value) and |d1|, |d2|, |d3| <= u; Ax, b
  and q are exact.  To first order |t^ - t| <= LOG*2u*b*ell + u*b*ell + u*(b*ell + Ax) + u*(b*ell + Ax + b)
  <= LOG*2u*b*ell + 3u*(b*ell + Ax + b); what the last step gives away, u*(Ax + 2b), is far more than the products of
  two d's.  poisson_fsum_kernel adds the t_i on a fixed tree: 1024 lanes of at most ceil(m/1024) terms, six levels of
  a wave sum, 16 partials in sequence -- never more than m + 16 roundings on the way of one term.  Hence

    |f - f_ref| <= sum_i [ LOG*2u*b_i*ell_i + 3u*(b_i*ell_i + Ax_i + b_i) ] + gamma_(m+16) * sum_i |t_i|.

  KL f.  t = ((Ax*lg)(1 + d1) - Ax)(1 + d2) + b, the same chain with Ax*ell in the place of b*ell:

    |f - f_ref| <= sum_i [ LOG*2u*Ax_i*ell_i + 3u*(Ax_i*ell_i + Ax_i + b_i) ] + gamma_(m+16) * sum_i |t_i|.

  KL g.  r^_i = r_i (1 + d0).  A column's sum is a chain of fma(r_i, A_ij, acc) (one rounding each) over the at most
  ceil(m/nsplit) rows of a split, then a sequential sum of nsplit <= 64 partials: at most m + 64 roundings.  With one
  more u to spare for second-order terms

    |g_j - g_ref,j| <= (LOG*2u + u + gamma_(m+64)) * sum_i A_ij*|r_i|.

The np.longdouble reference (64-bit significand) sums m terms with an error below m*2^-64 of the same sums of
magnitudes, 2^-11 of the gamma term of each bound.

LOG, the allowance for log in ulps, is measured, not derived.  NumPy's fp64 log against the np.longdouble log on the
quotients used here, {1/4, 1/2, 3/4, 1, 5/4, 3/2, 2, 4}: at most 0.470 ulp (at 3/4; log(1) = 0 is exact).  Rounded up
to a whole ulp, 1, plus one ulp for a different math library: LOG = 2.  test_poisson_forms_cpu.py repeats the
measurement and holds the fp64 NumPy formulas below every bound at every shape of the GPU module.

Shapes.  m is written (k, o) for k*CU + o where it depends on the compute-unit count of the device (256 on MI355X),
which the GPU module reads at run time and the host tests set to 256."""
import numpy as np

U = 2.0 ** -53
LOG_MEASURED = 0.470          # NumPy fp64 log against np.longdouble log on QUOTIENTS, in ulps
LOG = 2                       # ceil(LOG_MEASURED) + 1
P_POISSON = (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0)
P_KL = (0.25, 0.5, 1.0, 2.0, 4.0)
QUOTIENTS = (0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 4.0)
LD = np.longdouble

VG_COLS = 512                 # columns per workgroup of the split-row pass (fw_kernels.hip: 2 * FB)
VG_MAXSPLIT = 64


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------------- the data
def _exact(m, n, seed, pset, p_all_one):
    rng = np.random.RandomState(seed)
    A = rng.randint(1, 9, size=(m, n)).astype(np.float64)
    x = rng.randint(1, 257, size=n) / 64.0
    p = np.ones(m) if p_all_one else rng.choice(pset, size=m)
    b = A.dot(x) * p
    return A, x, p, b


def exact_poisson(m, n, seed, p_all_one=False):
    """(A, x, p, b) with b/(A x) == p exactly"""
    return _exact(m, n, seed, P_POISSON, p_all_one)


def exact_kl(m, n, seed, p_all_one=False):
    """(A, x, p, b) with (A x)/b == 1/p exactly"""
    return _exact(m, n, seed, P_KL, p_all_one)


def measure_log():
    """the largest error of NumPy's fp64 log on QUOTIENTS against the np.longdouble log, in ulps of the fp64 result"""
    worst = 0.0
    for q in QUOTIENTS:
        l64 = np.log(np.float64(q))
        if l64 == 0.0:
            assert q == 1.0
            continue
        worst = max(worst, float(abs(LD(l64) - np.log(LD(q))) / LD(np.spacing(abs(l64)))))
    return worst


# ------------------------------------------------------------------------------------------- the launch forms, copied
def vt_nsplit(m, n, cu):
    """vt_nsplit of fw_kernels.hip: the row splits of pass 2"""
    cb = (n + VG_COLS - 1) // VG_COLS
    s = (4 * cu // 5 + cb // 2) // cb
    s = min(s, VG_MAXSPLIT, m // 8)
    return max(s, 1)


def empty_splits(m, nsplit):
    """the splits of fw_vgemv_partial_body that own no row"""
    rows_per = (m + nsplit - 1) // nsplit
    return [s for s in range(nsplit) if s * rows_per >= m]


def ax_form(m, n, cu):
    """launch_ax of poisson_kernels.hip: "wg" a workgroup per row, "wave" a wavefront per row, "hold" a wavefront per
    row with the LDS request"""
    if m < 8 * cu and n >= 4096:
        return "wg"
    return "hold" if n >= 32768 else "wave"


def loads_16(n, lda, a_skew, x_skew):
    """(vec_ok of the handle, xvec of a call): 16-byte loads in pass 2, in pass 1"""
    vec_ok = (not a_skew) and lda % 2 == 0
    return vec_ok, vec_ok and not x_skew


def rows(shape, cu):
    (k, o), n = (shape[0], shape[1]) if isinstance(shape[0], tuple) else ((0, shape[0]), shape[1])
    return k * cu + o, n


# host-drawn shapes: (m, n), m = (k, o) for k*CU + o
HOST_SHAPES = [(1, 1), (3, 2), (4, 64), (5, 65), (7, 129), ((8, 2), 130), (33, 4096), (5, 4097), (33, 4095),
               (416, 1540), (520, 130), (1023, 3), (1024, 3), (1025, 3), (70001, 3)]
# device-drawn shapes: (m, n, lda)
DEVICE_SHAPES = [((8, -1), 4096, 4096), ((8, 0), 4096, 4096), ((8, 0), 32768, 32768), ((8, 0), 32767, 32768)]
# (m, n, lda - n, A base at 8 mod 16, x at 8 mod 16)
STRIDE_CASES = [
    (5, 65, 1, False, False), (7, 129, 3, False, False), (5, 4097, 1, False, False),       # even lda, odd n: the tail
    (5, 65, 2, False, False), (33, 4096, 5, False, False),                                 # odd lda: scalar loads
    (4, 64, 0, True, False), (5, 65, 1, True, False), (33, 4096, 2, True, False),          # A at 8 mod 16, even lda
    (4, 64, 0, False, True), (7, 129, 3, False, True), (33, 4096, 0, False, True),         # x at 8 mod 16
    ((8, 2), 130, 0, False, True),
]
NONFINITE_SHAPES = [(5, 65), (33, 4096)]
FLAG_SHAPES = [(7, 129), (33, 4096)]


def all_shapes(cu):
    """every (m, n) the GPU module runs"""
    out = [rows(s, cu) for s in HOST_SHAPES] + [rows(s, cu) for s in DEVICE_SHAPES]
    out += [rows(s, cu) for s in STRIDE_CASES] + NONFINITE_SHAPES + FLAG_SHAPES
    seen = []
    for s in out:
        if s not in seen:
            seen.append(s)
    return seen


# ------------------------------------------------------------------------------------------- the reference's formulas
def poisson_fp64(A, x, b):
    """(f, g, A x) as accbpg/functions.py:104-120 computes them in float64"""
    m = A.shape[0]
    with np.errstate(all="ignore"):
        Ax = np.dot(A, x)
        g = ((1 - b / Ax).reshape(m, 1) * A).sum(axis=0)
        fx = sum(b * np.log(b / Ax) + Ax - b)
    return fx, g, Ax


def kl_fp64(A, x, b):
    """(f, g, A x) as accbpg/functions.py:142-158 computes them in float64"""
    m = A.shape[0]
    with np.errstate(all="ignore"):
        Ax = np.dot(A, x)
        g = (np.log(Ax / b).reshape(m, 1) * A).sum(axis=0)
        fx = sum(Ax * np.log(Ax / b) - Ax + b)
    return fx, g, Ax


def poisson_terms(Ax, b):
    """np.longdouble (t, per-row allowance) of the Poisson value"""
    Ax, b = np.asarray(Ax, dtype=LD), np.asarray(b, dtype=LD)
    lg = np.log(b / Ax)
    ell = np.abs(lg)
    return b * lg + Ax - b, LOG * 2 * U * b * ell + 3 * U * (b * ell + Ax + b)


def kl_terms(Ax, b):
    """np.longdouble (t, per-row allowance) of the KL value"""
    Ax, b = np.asarray(Ax, dtype=LD), np.asarray(b, dtype=LD)
    lg = np.log(Ax / b)
    ell = np.abs(lg)
    return Ax * lg - Ax + b, LOG * 2 * U * Ax * ell + 3 * U * (Ax * ell + Ax + b)


def f_ref_and_bound(terms, Ax, b):
    """(f_ref, bound on |f - f_ref|) from the length-m vectors A x and b; terms is poisson_terms or kl_terms"""
    t, per = terms(Ax, b)
    m = t.size
    return np.sum(t), np.sum(per) + gamma(m + 16) * np.sum(np.abs(t))


def poisson_g_ref(A, Ax, b):
    """np.longdouble A^T (1 - b/Ax)"""
    r = 1 - np.asarray(b, dtype=LD) / np.asarray(Ax, dtype=LD)
    return r.dot(np.asarray(A, dtype=LD))


def kl_g_ref_and_bound(A, Ax, b):
    """np.longdouble (A^T log(Ax/b), bound on |g - g_ref|)"""
    r = np.log(np.asarray(Ax, dtype=LD) / np.asarray(b, dtype=LD))
    Al = np.asarray(A, dtype=LD)
    m = Al.shape[0]
    return r.dot(Al), (LOG * 2 * U + U + gamma(m + 64)) * np.abs(r).dot(np.abs(Al))


def kl_g_ref_and_bound_grouped(S, m):
    """The same from S[k] = sum of the rows of A with p_i = P_KL[k] (exact in float64): r takes the five values
    log(1/P_KL[k]), so A^T r = sum_k log(1/P_KL[k]) S[k] needs no pass over A in np.longdouble."""
    r = np.log(1 / np.asarray(P_KL, dtype=LD))
    Sl = np.asarray(S, dtype=LD)
    return r.dot(Sl), (LOG * 2 * U + U + gamma(m + 64)) * np.abs(r).dot(Sl)


def group_sums(A, p):
    return np.stack([A[p == pk].sum(axis=0) for pk in P_KL])


def classes(v):
    """0 finite, 1 +inf, 2 -inf, 3 NaN, entry by entry"""
    v = np.atleast_1d(np.asarray(v, dtype=np.float64))
    return np.where(np.isnan(v), 3, np.where(v == np.inf, 1, np.where(v == -np.inf, 2, 0)))
