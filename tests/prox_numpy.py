"""Vectorised NumPy restatement of the Burg simplex prox (accbpg/functions.py:336-356 with :264-271 in front), the
forward error bound of each launch form of csrc/vec_kernels.hip, and the cases that tests/test_gpu_prox.py runs on the
device and tests/test_prox_cpu.py validates on the host.

Launch forms (`variant`, the codes of accbpg_debug_prox_state):
   10, 11, 12   burg_prox_kernel<2>, <8>, <32>      one workgroup of 1024 threads, gg in registers
    1           burg_prox_kernel<0>                 one workgroup, gg re-read from the workspace
    2, 3        burg_prox_multi_kernel<8>, <32>     ceil(n / (1024*EPT)) workgroups, partial sums exchanged

No bound below holds a measured number: u = 2^-53, the depths are read off the code (line references at `depth`), the
factors are stated with their reason.
"""
import numpy as np

U = 2.0 ** -53                # unit roundoff of float64
PB = 1024                     # threads of a prox workgroup (vec_kernels.hip: `constexpr int PB = 1024`)
EPT = {10: 2, 11: 8, 12: 32, 2: 8, 3: 32}
MAX_STEPS = 4096              # cap of either loop in the kernels (`nb < 4096`, `nn < 4096`)
MSG = "Either y or L is not positive."          # functions.py:270

assert np.finfo(np.longdouble).nmant >= 63, "the reference replay needs an extended-precision long double"


def by_size(n):
    """the form production dispatch selects (accbpg_burg_simplex_div_prox, latch clear)"""
    if n <= PB * 2:
        return 10
    if n <= PB * 8:
        return 11
    if n <= PB * 32:
        return 12
    if n <= PB * 8 * 128:
        return 2
    if n <= PB * 32 * 128:
        return 3
    return 1


def workgroups(variant, n):
    return -(-n // (PB * EPT[variant])) if variant in (2, 3) else 1


def make_gg(y, g, L):
    """gg of functions.py:341 behind :271 and :248: (g - L*(-1/y))/L, or g/L without y.  One correctly rounded float64
    operation per ufunc, the operations of make_gg in burg_prox_body and of the load loop of burg_prox_multi_kernel
    (built with -ffp-contract=off): bit for bit the kernel's gg."""
    g = np.asarray(g, dtype=np.float64)
    L = np.float64(L)
    if y is None:
        return g / L
    with np.errstate(divide="ignore", invalid="ignore"):
        t = -1.0 / np.asarray(y, dtype=np.float64)
        return (g - L * t) / L


class Replay:
    """iterates of one replay: c[k], phi[k], dphi[k] (phi' at c[k]), S[k] = sum |1/(gg + c[k])|; k = 0 is the start
    c = cmin + 1 after `nb` bisections, k = nn the returned point.  `stalled`: left by the test of :351-352."""


def replay(gg, eps, dtype):
    """functions.py:336-356 on a given gg with array sums in `dtype` (the sums of np.sum are pairwise)."""
    gg = np.asarray(gg).astype(dtype)
    one = dtype(1)

    def phi(c):
        r = one / (gg + c)
        return r.sum() - one, np.abs(r).sum()

    def dphi(c):
        r = gg + c
        return (-one / (r * r)).sum()

    R = Replay()
    with np.errstate(all="ignore"):
        cmin = -gg.min()                                  # :342 (np.min keeps a NaN)
        c = cmin + one                                    # :344
        nb = nn = 0
        f, S = phi(c)
        while f < 0 and nb < MAX_STEPS:                   # :345-346
            c = (cmin + c) / dtype(2)
            f, S = phi(c)
            nb += 1
        R.c, R.phi, R.S, R.dphi = [c], [f], [S], []
        R.stalled = False
        while abs(f) > eps and nn < MAX_STEPS:            # :349
            d = dphi(c)                                   # :350
            R.dphi.append(d)
            step = f / d
            if (c - (c - step)) == 0:                     # :351-352
                R.stalled = True
                break
            c = c - step                                  # :353
            f, S = phi(c)                                 # :354
            nn += 1
            R.c.append(c); R.phi.append(f); R.S.append(S)
        if len(R.dphi) < len(R.c):
            R.dphi.append(dphi(c))
        R.nb, R.nn = nb, nn
        R.x = one / (gg + c)                              # :355
    return R


def depth(variant, n):
    """Longest chain of additions behind one value of phi in that form (vec_kernels.hip):
      per thread   `for e < EPT: s += 1.0 / (gg[e] + c)` in phi of burg_prox_body and in `both` of
                   burg_prox_multi_kernel: EPT additions (entries past n add an exact 0.0);
                   `for (i = tid; i < n; i += PB) s += ...` of the EPT == 0 form: ceil(n / 1024)
      wave         wave_sum (reduce.hpp): `for off = 32 .. 1: v += __shfl_down(v, off)`: 6
      workgroup    block_sum_bcast: `for i < PB/64: s += sh[i]`: 16
      multi forms  pm_exchange<0>: `for v = 1 .. G-1: sa += pa`: at most G, the workgroup count."""
    per_thread = -(-n // PB) if variant == 1 else EPT[variant]
    d = per_thread + 6 + 16
    if variant in (2, 3):
        d += workgroups(variant, n)
    return d


def phi_err(variant, n, S):
    """|phi the kernel computes at c  -  phi(c)| <= (d + 3) u S + u, with S = sum |1/(gg_i + c)|.
    Each term carries two roundings (the sum gg_i + c, the division) and at most d of the additions:
    (1 + u)^(d+2) - 1 <= (d + 2) u to first order, times S.  The final `- 1.0` rounds once more: u |s - 1| <= u S + u.
    Second-order terms ((d + 2)^2 u^2 S, d <= 4119 here) are 12 decades below and left out."""
    return (depth(variant, n) + 3) * U * float(S) + U


def c_quantum(c, dphi):
    """u |c| |phi'(c)|: what rounding c to float64 moves phi by.  The stall test of :351-352 leaves the loop once
    |step| <= half an ulp of c <= u |c|, i.e. |phi| <= u |c| |phi'| (the computed phi' is within 2^-40 relative of
    the exact one, d + 6 roundings; 2^-30 covers that and the rounding of the quotient)."""
    return U * abs(float(c)) * abs(float(dphi)) * (1.0 + 2.0 ** -30)


def stall_regime(R, eps):
    """True where the float64 loop may stop by the stall test instead of |phi| <= eps: the reference itself stalled, or
    one float64 step of c moves phi by eps or more.  A property of the input, taken from the reference alone.
    Below it a float64 loop that still has |phi| > eps takes a step longer than u |c| and so cannot stall."""
    return bool(R.stalled or c_quantum(R.c[-1], R.dphi[-1]) >= eps)


def count_margin_ok(R, eps, variant, n):
    """The condition of the count comparison: no iterate of the reference has |phi_k| within
    4 (phi_err(k) + u |c_k| |phi'_k|) of eps.  (The kernel's iterate k differs from the reference's by the last step's
    rounding only -- Newton contracts what came before quadratically -- which moves phi by at most
    phi_err + u |c| |phi'|, and its own evaluation adds phi_err.)"""
    for c, f, S, d in zip(R.c, R.phi, R.S, R.dphi):
        if abs(abs(float(f)) - eps) <= 4.0 * (phi_err(variant, n, S) + c_quantum(c, d)):
            return False
    return True


def c_bound(R, variant, n):
    """|c_kernel - c_R| <= 8 (phi_err / |phi'_R(c_R)| + u |c_R|): the last step's rounding, with 8 as margin for the
    neglected second-order term."""
    return 8.0 * (phi_err(variant, n, R.S[-1]) / abs(float(R.dphi[-1])) + U * abs(float(R.c[-1])))


def phi_at(gg, c):
    """phi in long double at a float64 c: (phi, S, phi')"""
    r = np.longdouble(1) / (gg.astype(np.longdouble) + np.longdouble(c))
    return r.sum() - np.longdouble(1), np.abs(r).sum(), -(r * r).sum()


def recover_c(gg, x, near=None):
    """The kernels write x_i = 1.0 / (gg_i + c) with two IEEE operations, so one float64 c reproduces a whole output
    bit for bit.  Entry i admits the c for which gg_i + c rounds into the run of doubles r with fl(1/r) == x_i: an
    interval, formed in long double from the midpoints at either end of that run.  The doubles in the intersection of
    all intervals are then tried for what they are: a candidate counts only if it reproduces every entry exactly.  At
    most 8 doubles either way of the starting point are tried: `near` (default: the middle) clipped into the
    intersection.  Where neighbouring doubles reproduce the output equally (they are then the same result), the one
    closest to the starting point is returned.  ValueError if no c reproduces every entry.

    (1/x_k - gg_k at the smallest gg alone is no usable starting point: where |c| is small against gg_k + c, its
    error, an ulp of gg_k + c, is many doubles of c.)"""
    gg = np.asarray(gg, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)
    if gg.shape != x.shape or gg.ndim != 1:
        raise ValueError("recover_c: shapes differ")
    ld = np.longdouble
    fin = np.isfinite(gg)                                 # an entry with gg = inf gives 0.0 for every c
    with np.errstate(all="ignore"):
        if not np.array_equal(x[~fin], np.float64(1.0) / gg[~fin]):
            raise ValueError("recover_c: no single c reproduces the output")
        g1, x1 = gg[fin], x[fin]
        if g1.size == 0 or not np.all(np.isfinite(x1)) or np.any(x1 == 0):
            raise ValueError("recover_c: no finite c")
        r = np.float64(1.0) / x1
        rs = [r]
        for _ in range(3):
            rs = [np.nextafter(rs[0], -np.inf)] + rs + [np.nextafter(rs[-1], np.inf)]
        ok = [np.float64(1.0) / q == x1 for q in rs]
        if not np.all(np.any(ok, axis=0)):
            raise ValueError("recover_c: an entry is no reciprocal of a double")
        r_lo = np.min(np.where(ok, rs, np.inf), axis=0)
        r_hi = np.max(np.where(ok, rs, -np.inf), axis=0)
        lo = ((r_lo.astype(ld) + np.nextafter(r_lo, -np.inf).astype(ld)) / 2 - g1.astype(ld)).max()
        hi = ((r_hi.astype(ld) + np.nextafter(r_hi, np.inf).astype(ld)) / 2 - g1.astype(ld)).min()
        start = (lo + hi) / 2 if near is None else ld(near)
        c0 = np.float64(min(max(start, lo), hi))
        up = dn = c0
        cands = [c0]
        for _ in range(8):
            up = np.nextafter(up, np.inf)
            dn = np.nextafter(dn, -np.inf)
            cands += [up, dn]
        probe = np.unique(np.linspace(0, gg.size - 1, 64).astype(np.int64))
        for c in cands:
            if not np.array_equal(np.float64(1.0) / (gg[probe] + c), x[probe]):
                continue
            if np.array_equal(np.float64(1.0) / (gg + c), x):
                return float(c)
    raise ValueError("recover_c: no single c reproduces the output")


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
FORCED = [(1, 1), (1, 1025), (1, 5000), (1, 40000),
          (2, 8193), (2, 40000), (2, 3 * 8192),
          (3, 32769), (3, 3 * 32768 - 7), (3, 5 * 32768)]
PRODUCTION = [(0, n) for n in (1, 2048, 2049, 8192, 8193, 32768)]
# data: (family, L, eps)
DATA = [("random", 1.0, 1e-8), ("random", 0.02, 1e-8), ("equal", 1.0, 1e-8), ("vertex", 1.0, 1e-8),
        ("mixed", 1.0, 1e-8), ("random", 1.0, 1e-6), ("random", 1.0, 1e-12)]
CASES = [(v, n, fam, L, eps, form) for (v, n) in FORCED + PRODUCTION for (fam, L, eps) in DATA
         for form in ("div", "prox")]
THRESHOLDS = [(32768, 12), (32769, 2), (1048576, 2), (1048577, 3), (4194304, 3), (4194305, 1)]


def case_id(case):
    v, n, fam, L, eps, form = case
    return "v%d-n%d-%s-L%g-eps%g-%s" % (v, n, fam, L, eps, form)


def launched(variant, n):
    """the form a call under accbpg_debug_prox_variant(variant) launches"""
    return variant if variant else by_size(n)


def random_family(n, seed):
    """the family of test_prox_sizes_against_oracle"""
    rng = np.random.RandomState(seed)
    y = rng.rand(n) + 1e-3
    y /= y.sum()
    g = -rng.rand(n) * 50 - 1
    return y, g


def inputs(n, fam, L, form):
    """(y or None, g) of a case.  The prox_map form takes the argument the div form builds, computed on the host."""
    if fam == "random":
        y, g = random_family(n, n)
    elif fam == "equal":                                  # a tie of all entries: Newton from phi = n - 1, result 1/n
        y = np.full(n, 1.0 / n)
        g = np.full(n, -3.0)
    elif fam == "vertex":                                 # one entry below the rest by 1e9 L
        y, g = random_family(n, n + 1)
        g[(7 * n) // 11] -= 1e9 * L
    elif fam == "mixed":                                  # late BPG iterates: a tenth of y at 1e-12/n
        y, g = random_family(n, n + 2)
        small = np.arange(n) % 10 == 3
        y[small] = 1e-12 / n
        y[~small] *= (1.0 - y[small].sum()) / y[~small].sum()
    else:
        raise ValueError(fam)
    if form == "prox":
        return None, g + L / y
    return y, g
