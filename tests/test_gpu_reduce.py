"""GPU tests of the fixed reduction tree of the length-n kernels (csrc/reduce.hpp) through the public
wrappers, at the sizes where the tree changes shape (reduce_numpy.edge_sizes: one lane / wave / block, nb 1 -> 2, 256
-> 257 records in the final stage, the block cap and one entry past it, a ragged multi-trip size) for the caps 1024
(vec_, inexact_kernels.hip), 512 (shannon_, quartic_kernels.hip) and 128 (accbpg_vec_argminmax).

(a) Bit equality with the emulator tests/reduce_numpy.py for every slot whose term is built from + - * / on float64.
    csrc/Makefile compiles vec_, fw_, poisson_, shannon_, symnmf_, quartic_ and inexact_kernels with
    -ffp-contract=off; dopt_kernels, capi, batch and shard are not, and none of those holds a length-n reduction
    tested here, so every slot below is held bit-equal, products included.  shannon_ls_terms returns
    o1 + (Sy - Sx): Sy (and Sz1) is read out bit for bit with x = 0 (z = 0), where o1 = Sx = 0; Sx has no such
    handle and enters through (b) and (d) only.
(b) Integer-valued inputs, exact in any order: every kernel of (a) must return the integer; one outlier planted in
    constant data at the seams of the tree (reduce_numpy.planted_positions).
(c) vec_argminmax: first index among ties across lanes, waves, blocks and trips; a NaN is both extrema.
(d) Log-bearing sums against math.fsum over terms formed in np.longdouble, within
    (tree_depth + k) * eps * sum_i M_i, M_i the magnitudes of the intermediates of term i, k one per rounding plus
    the device log / exp error in ulps.  No accuracy table of the HIP math library is installed with ROCm here, so
    the figure is measured (fixture `ulps`): log through ShannonEntropy.gradient = 1 + log r on the test's own ratios
    that lie in [0.14, 0.6], where 1 + log r is exact (Sterbenz) and the device logarithm is recovered bit for bit;
    exp through ShannonEntropy.prox_map on arguments -g - 1 that are exact; one ulp of margin is added to each.
    Measured on the MI355X (printed by the fixture): log 0.534 ulp over 142469 ratios, exp 0.837 ulp over 200001
    arguments, so the bounds use 1.534 and 1.837.
(e) NaN, 0.0 and a negative entry planted at the seams: the value of vec_min_sum, the AssertionError of the others.
(f) Interleaved 4-slot and 8-slot reductions share ws + n and the device scratch and repeat bit for bit; the two
    passes of lmo_l2_ball_positive_orthant.
(g) accbpg_dopt_batch_ls_terms equals the single-instance ls_terms bit for bit at n = 2**20 + 1.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_numpy as T  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = T.EPS
LD = np.longdouble
VEC_SIZES = T.edge_sizes(T.CAP_VEC)
WIDE_SIZES = T.edge_sizes(T.CAP_WIDE)
ARG_SIZES = T.edge_sizes(T.CAP_ARG)


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


_CACHE = {}


def data(n):
    """host vectors of length n, drawn once and never written: g, x, y, z, w of mixed sign, px .. pw positive, and
    ig .. iw small integers (|.| <= 8), pix .. piw positive integers (1 .. 9); `d` holds the device copies"""
    if n not in _CACHE:
        h = {}
        for k, name in enumerate("gxyzw"):
            v = T.draw(n, k)
            h[name] = v
            h["p" + name] = np.abs(v) + 0.05
            h["i" + name] = np.rint(np.clip(3.0 * v, -8, 8))
            h["pi" + name] = np.abs(h["i" + name]) + 1.0
        h["d"] = {k: dev(v) for k, v in h.items()}
        _CACHE[n] = h
    return _CACHE[n]


def fsum_ld(t):
    """the sum of longdouble terms, each split into two doubles so that fsum sees them exactly"""
    t = np.asarray(t, dtype=LD)
    hi = t.astype(np.float64)
    lo = (t - hi).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]))


def _lib_ws(t):
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import _Workspace, _ptr, _stream
    return _lib, _lib.load(), _ptr, _ptr(_Workspace.get(t.numel(), t.device)), _stream()


def quartic_prox_stage(y, g, z, invL, clip, ub):
    """the C entry behind SumOf2nd4thPowers.div_prox_map: (y', ||y'||^2)"""
    _lib, lib, _ptr, ws, stream = _lib_ws(y)
    out = torch.empty_like(y)
    ssq = C.c_double(0.0)
    rc = lib.accbpg_quartic_prox_stage(_ptr(y), _ptr(g), float(z), float(invL), int(clip), float(ub), y.numel(), _ptr(out),
                                       C.byref(ssq), ws, stream)
    _lib.check(rc, "accbpg_quartic_prox_stage")
    return out, ssq.value


def lmo_pos(g, c, radius, eps):
    """the C entry behind lmo_l2_ball_positive_orthant: (s, [count of g < 0, ||s - c||, min s])"""
    _lib, lib, _ptr, ws, stream = _lib_ws(g)
    out = torch.empty_like(g)
    info = (C.c_double * 3)()
    rc = lib.accbpg_lmo_l2_ball_pos(_ptr(g), _ptr(c), float(radius), float(eps), g.numel(), _ptr(out), info, ws, stream)
    _lib.check(rc, "accbpg_lmo_l2_ball_pos")
    return out, list(info)


class planted:
    """t[p] = value on the device for the length of the block, then the old entry again"""

    def __init__(self, t, p, value):
        self.t, self.p, self.value = t, p, value

    def __enter__(self):
        self.old = self.t[self.p].clone()
        self.t[self.p] = self.value
        return self.t

    def __exit__(self, *exc):
        self.t[self.p] = self.old
        return False


# =================================================================================================== (a) bit equality
@pytest.mark.parametrize("n", VEC_SIZES)
def test_bit_equal_vec_kernels(acc, n):
    from accbpg_and_fw_amd.functions import ls_terms, vec_dot, vec_dot_diff, vec_min_sum
    h = data(n)
    d = h["d"]
    cap = T.CAP_VEC
    assert vec_dot(d["x"], d["y"]) == T.tree_sum(h["x"] * h["y"], cap)
    assert vec_dot(d["x"], d["x"]) == T.tree_sum(h["x"] * h["x"], cap)
    mn, sm = vec_min_sum(d["x"])
    assert sm == T.tree_sum(h["x"], cap) and mn == h["x"].min() == T.tree_min(h["x"], cap)
    diff = h["x"] - h["y"]
    assert vec_dot_diff(d["g"], d["x"], d["y"]) == T.tree_sum(h["g"] * diff, cap)
    diff = h["px"] - h["py"]
    want = T.tree_sum(h["g"] * diff, cap)
    assert ls_terms(d["g"], d["px"], d["py"])[0] == want
    assert ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"])[0] == want


def _quartic_slots(h, g, x, y, z, w, cap=T.CAP_WIDE):
    x, y = h[x], h[y]
    dxy = x - y
    out = [T.tree_sum(h[g] * dxy, cap) if g else 0.0, T.tree_sum(x * x, cap), T.tree_sum(y * y, cap),
           T.tree_sum(y * dxy, cap)]
    if z:
        z, w = h[z], h[w]
        out += [T.tree_sum(z * z, cap), T.tree_sum(w * w, cap), T.tree_sum(w * (z - w), cap)]
    else:
        out += [0.0, 0.0, 0.0]
    return tuple(out)


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_bit_equal_quartic_kernels(acc, n):
    from accbpg_and_fw_amd.functions import quartic_ls_terms
    h = data(n)
    d = h["d"]
    assert quartic_ls_terms(d["g"], d["x"], d["y"], d["z"], d["w"]) == _quartic_slots(h, "g", "x", "y", "z", "w")
    assert quartic_ls_terms(None, d["x"], d["y"]) == _quartic_slots(h, None, "x", "y", None, None)
    assert quartic_ls_terms(d["g"], d["y"], d["x"]) == _quartic_slots(h, "g", "y", "x", None, None)
    # the prox stage: y' = z*y - invL*g (two products, one difference), then the sum of its squares
    zc, invL = 1.7, 0.37
    for clip, ub in ((0, np.inf), (1, 0.9)):
        out, ssq = quartic_prox_stage(d["y"], d["g"], zc, invL, clip, ub)
        a = zc * h["y"]
        b = invL * h["g"]
        v = a - b
        if clip:
            v = np.clip(v, 0.0, ub)
        np.testing.assert_array_equal(out.cpu().numpy(), v)
        assert ssq == T.tree_sum(v * v, T.CAP_WIDE)
    # through the class: x / z' with z' the cubic's root at alpha * ||y'||^2
    hq = acc.SumOf2nd4thPowers(alpha=0.3, sigma=0.8)
    got = hq.div_prox_map(d["y"], d["g"], 2.5)
    zc = 0.3 * np.sqrt(np.float64(T.tree_sum(h["y"] * h["y"], T.CAP_VEC))) ** 2 + 0.8
    a = float(zc) * h["y"]
    b = float(1 / 2.5) * h["g"]
    v = a - b
    root = hq.solve_cubic(0.3 * np.sqrt(np.float64(T.tree_sum(v * v, T.CAP_WIDE))) ** 2, 0.8)
    np.testing.assert_array_equal(got.cpu().numpy(), v / float(root))


@pytest.mark.parametrize("n", VEC_SIZES)
def test_bit_equal_combine_ls_terms(acc, n):
    from accbpg_and_fw_amd.functions import combine_ls_terms
    h = data(n)
    d = h["d"]
    a, b, c = 0.3, 0.7, 1.3
    for kernel, u, v, x in ((acc.SquaredL2Norm(), "x", "y", "z"), (acc.BurgEntropy(), "px", "py", "pz")):
        w, lin, dist = combine_ls_terms(kernel, a, d[u], b, d[v], c, d["g"], d[x])
        p = a * h[u]
        q = b * h[v]
        wr = (p + q) / c
        np.testing.assert_array_equal(w.cpu().numpy(), wr)
        diff = wr - h[x]
        # a single block writes the result itself: no final stage
        assert lin == T.tree_sum(h["g"] * diff, T.CAP_VEC, single_block_final=False)
        if isinstance(kernel, acc.SquaredL2Norm):
            assert dist == 0.5 * T.tree_sum(diff * diff, T.CAP_VEC, single_block_final=False)


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_bit_equal_shannon_add_only_slots(acc, n):
    from accbpg_and_fw_amd.functions import shannon_ls_terms
    h = data(n)
    d = h["d"]
    diff = h["px"] - h["py"]
    lin, dxy, dzz = shannon_ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"])
    assert lin == T.tree_sum(h["g"] * diff, T.CAP_WIDE)
    # x = 0 (accepted: the assertion is >= 0): every x*log term and sum x are 0, D = 0 + (sum y - 0)
    zero = torch.zeros_like(d["py"])
    lin, dxy, dzz = shannon_ls_terms(d["g"], zero, d["py"], zero, d["pw"])
    assert lin == T.tree_sum(h["g"] * (0.0 - h["py"]), T.CAP_WIDE)
    assert dxy == T.tree_sum(h["py"], T.CAP_WIDE) and dzz == T.tree_sum(h["pw"], T.CAP_WIDE)


# =================================================================================================== (b) exact coverage
@pytest.mark.parametrize("n", VEC_SIZES)
def test_exact_integers_vec_and_inexact(acc, n):
    from accbpg_and_fw_amd.functions import combine_ls_terms, ls_terms, vec_dot, vec_dot_diff, vec_min_sum
    h = data(n)
    d = h["d"]

    def exact(v):
        return float(int(np.sum(v)))

    assert vec_dot(d["ix"], d["iy"]) == exact(h["ix"] * h["iy"])
    assert vec_min_sum(d["ix"]) == (h["ix"].min(), exact(h["ix"]))
    assert vec_dot_diff(d["ig"], d["ix"], d["iy"]) == exact(h["ig"] * (h["ix"] - h["iy"]))
    assert ls_terms(d["ig"], d["pix"], d["piy"])[0] == exact(h["ig"] * (h["pix"] - h["piy"]))
    for kernel, u, v, x in ((acc.SquaredL2Norm(), "ix", "iy", "iz"), (acc.BurgEntropy(), "pix", "piy", "piz")):
        w, lin, dist = combine_ls_terms(kernel, 2.0, d[u], 3.0, d[v], 1.0, d["ig"], d[x])
        wr = 2.0 * h[u] + 3.0 * h[v]
        np.testing.assert_array_equal(w.cpu().numpy(), wr)
        assert lin == exact(h["ig"] * (wr - h[x]))
        if isinstance(kernel, acc.SquaredL2Norm):
            assert dist == 0.5 * exact((wr - h[x]) ** 2)
    # one outlier in constant data
    c3 = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    c2 = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
    c1 = torch.ones(n, dtype=torch.float64, device="cuda")
    for p in T.planted_positions(n, T.CAP_VEC):
        with planted(c3, p, 1003.0):
            assert vec_min_sum(c3) == (3.0 if n > 1 else 1003.0, 3.0 * n + 1000.0), p
            assert vec_dot(c3, c2) == 6.0 * n + 2000.0, p
            assert vec_dot_diff(c2, c3, c1) == 4.0 * n + 2000.0, p
            assert ls_terms(c2, c3, c1)[0] == 4.0 * n + 2000.0, p
            w, lin, dist = combine_ls_terms(acc.SquaredL2Norm(), 1.0, c3, 1.0, c1, 1.0, c2, c1)     # w = c3 + c1
            assert lin == 6.0 * n + 2000.0 and dist == 0.5 * (9.0 * (n - 1) + 1003.0 ** 2), p
        with planted(c3, p, 0.5):                  # the unique minimum, positive: a final stage started at 0 shows
            assert vec_min_sum(c3) == (0.5, 3.0 * n - 2.5), p
        with planted(c3, p, -1000.0):
            assert vec_min_sum(c3) == (-1000.0, 3.0 * n - 1003.0), p


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_exact_integers_quartic_and_shannon(acc, n):
    from accbpg_and_fw_amd.functions import quartic_ls_terms, shannon_ls_terms
    h = data(n)
    d = h["d"]

    def exact(v):
        return float(int(np.sum(v)))

    ig, ix, iy, iz, iw = (h[k] for k in ("ig", "ix", "iy", "iz", "iw"))
    want = (exact(ig * (ix - iy)), exact(ix * ix), exact(iy * iy), exact(iy * (ix - iy)), exact(iz * iz),
            exact(iw * iw), exact(iw * (iz - iw)))
    assert quartic_ls_terms(d["ig"], d["ix"], d["iy"], d["iz"], d["iw"]) == want
    assert quartic_ls_terms(None, d["ix"], d["iy"]) == (0.0,) + want[1:4] + (0.0, 0.0, 0.0)
    out, ssq = quartic_prox_stage(d["iy"], d["ig"], 3.0, 2.0, 0, np.inf)
    v = 3.0 * iy - 2.0 * ig
    np.testing.assert_array_equal(out.cpu().numpy(), v)
    assert ssq == exact(v * v)
    zero = torch.zeros(n, dtype=torch.float64, device="cuda")
    lin, dxy, dzz = shannon_ls_terms(d["ig"], zero, d["piy"], zero, d["piw"])
    assert (lin, dxy, dzz) == (exact(-ig * h["piy"]), exact(h["piy"]), exact(h["piw"]))
    # x == y: every logarithm is log(1) = 0 and sum y - sum x cancels exactly, whatever the order
    lin, dxy, dzz = shannon_ls_terms(d["ig"], d["pix"], d["pix"], d["piz"], d["piz"])
    assert (lin, dxy, dzz) == (0.0, 0.0, 0.0)
    c3 = torch.full((n,), 3.0, dtype=torch.float64, device="cuda")
    c2 = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
    for p in T.planted_positions(n, T.CAP_WIDE):
        with planted(c3, p, 1003.0):
            sq = 9.0 * (n - 1) + 1003.0 ** 2
            cross = 2.0 * n + 2000.0                                       # <c2, c3 - c2>
            assert quartic_ls_terms(c2, c3, c2, c3, c2) == (cross, sq, 4.0 * n, cross, sq, 4.0 * n, cross), p
            assert quartic_ls_terms(c2, c2, c3)[:4] == (-cross, 4.0 * n, sq, -(3.0 * (n - 1) + 1003.0 * 1001.0)), p
            out, ssq = quartic_prox_stage(c3, c2, 1.0, 1.0, 0, np.inf)     # y' = c3 - c2
            assert ssq == 1.0 * (n - 1) + 1001.0 ** 2, p
            lin, dxy, dzz = shannon_ls_terms(c2, zero, c3, zero, c3)
            assert (lin, dxy, dzz) == (-(6.0 * n + 2000.0), 3.0 * n + 1000.0, 3.0 * n + 1000.0), p


# =================================================================================================== (c) arg-min/max
@pytest.mark.parametrize("n", ARG_SIZES)
def test_argminmax_ties_and_nan(acc, n):
    from accbpg_and_fw_amd.functions import vec_argminmax
    h = data(n)
    x = h["x"]
    assert vec_argminmax(h["d"]["x"]) == (int(np.argmin(x)), int(np.argmax(x)), x.min(), x.max())
    c = torch.full((n,), 2.0, dtype=torch.float64, device="cuda")
    assert vec_argminmax(c) == (0, 0, 2.0, 2.0)                           # all equal: the first index
    pos = T.planted_positions(n, T.CAP_ARG)
    pairs = list(zip(pos[:-1], pos[1:])) + [(pos[0], pos[-1])] if len(pos) > 1 else []
    for p in pos:
        with planted(c, p, -5.0):                                         # the maximum: the first of the others
            assert vec_argminmax(c) == ((p, 0 if p else 1, -5.0, 2.0) if n > 1 else (0, 0, -5.0, -5.0)), p
        with planted(c, p, 9.0):
            assert vec_argminmax(c)[1::2] == (p, 9.0), p
        with planted(c, p, float("nan")):
            imin, imax, vmin, vmax = vec_argminmax(c)
            assert (imin, imax) == (p, p) and np.isnan(vmin) and np.isnan(vmax), p
    for p, q in pairs:                                                    # ties across the seams: the first wins
        with planted(c, p, -5.0), planted(c, q, -5.0):
            assert vec_argminmax(c)[0::2] == (p, -5.0), (p, q)
        with planted(c, p, 9.0), planted(c, q, 9.0):
            assert vec_argminmax(c)[1::2] == (p, 9.0), (p, q)
        with planted(c, p, float("nan")), planted(c, q, float("nan")):
            assert vec_argminmax(c)[:2] == (p, p), (p, q)
        with planted(c, p, -5.0), planted(c, q, float("nan")):            # a NaN beats a smaller value before it
            assert vec_argminmax(c)[:2] == (q, q), (p, q)


# =================================================================================================== (d) log-bearing sums
@pytest.fixture(scope="module")
def ulps(acc):
    """(log, exp) error of the device in ulps, measured as the module docstring says, plus one ulp of margin each"""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    h = data(T.CAP_WIDE * T.PER_BLOCK + 1)
    r = h["px"] / h["py"]
    r = r[(r >= 0.14) & (r <= 0.6)]
    assert r.size > 10000
    grad = acc.ShannonEntropy().gradient(r)                              # 1 + log r, exact for log r in [-2, -1/2]
    lg = grad - 1.0
    ref = np.log(r.astype(LD))
    u_log = float(np.max(np.abs(lg.astype(LD) - ref) / np.spacing(np.abs(ref.astype(np.float64))).astype(LD)))
    g = np.rint(T.draw(200001, 9) * 2.0 ** 28) / 2.0 ** 30                # multiples of 2**-30, |g| < 2: -g - 1 exact
    ex = acc.ShannonEntropy().prox_map(g, 1.0)
    ref = np.exp((-g - 1.0).astype(LD))
    u_exp = float(np.max(np.abs(ex.astype(LD) - ref) / np.spacing(ref.astype(np.float64)).astype(LD)))
    print("device log %.3f ulp over %d ratios, exp %.3f ulp over %d arguments" % (u_log, r.size, u_exp, g.size))
    assert u_log < 4 and u_exp < 4                                        # a measurement gone wrong, not a bound
    return u_log + 1.0, u_exp + 1.0


def _burg(xs, ys):
    """(fsum of x/y - log(x/y) - 1 in longdouble, sum of the magnitudes |r| + |log r| + 1)"""
    r = xs.astype(LD) / ys.astype(LD)
    lg = np.log(r)
    return fsum_ld(r - lg - 1), fsum_ld(np.abs(r) + np.abs(lg) + 1)


@pytest.mark.parametrize("n", VEC_SIZES)
def test_burg_log_sums_within_the_depth_bound(acc, ulps, n):
    """term = (r - log r) - 1 with r = x/y: a division, two subtractions (3 roundings) and the device log"""
    from accbpg_and_fw_amd.functions import combine_ls_terms, ls_terms
    h = data(n)
    d = h["d"]
    k = 3 + ulps[0]
    dxy, mxy = _burg(h["px"], h["py"])
    dzw, mzw = _burg(h["pz"], h["pw"])
    depth = T.tree_depth(n, T.CAP_VEC)
    lin, got_xy, got_zw = ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"])
    div = acc.BurgEntropy().divergence(d["px"], d["py"])
    print("n %d depth %d  D(x,y) err %.3e bound %.3e  D(z,w) err %.3e bound %.3e" % (
        n, depth, abs(got_xy - dxy), (depth + k) * EPS * mxy, abs(got_zw - dzw), (depth + k) * EPS * mzw))
    assert abs(got_xy - dxy) <= (depth + k) * EPS * mxy
    assert abs(got_zw - dzw) <= (depth + k) * EPS * mzw
    assert div == got_xy                                                  # the same pass without g and z
    w, lin, dist = combine_ls_terms(acc.BurgEntropy(), 0.3, d["px"], 0.7, d["py"], 1.3, d["g"], d["pz"])
    ref, mag = _burg(w.cpu().numpy(), h["pz"])
    depth = T.tree_depth(n, T.CAP_VEC, single_block_final=False)
    print("n %d combine depth %d err %.3e bound %.3e" % (n, depth, abs(dist - ref), (depth + k) * EPS * mag))
    assert abs(dist - ref) <= (depth + k) * EPS * mag


def _shannon(xs, ys, delta):
    """(S1 + (Sy - Sx) in longdouble, sum of the magnitudes |x|(|log| + 1) + |x| + |y|)"""
    xl, yl = xs.astype(LD), ys.astype(LD)
    lg = np.log((xl + LD(delta)) / (yl + LD(delta)))
    ref = LD(fsum_ld(xl * lg)) + (LD(math.fsum(ys)) - LD(math.fsum(xs)))
    return float(ref), fsum_ld(np.abs(xl) * (np.abs(lg) + 1) + np.abs(xl) + np.abs(yl))


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_shannon_divergences_within_the_depth_bound(acc, ulps, n):
    """term = x * log((x+delta)/(y+delta)): two sums, a division, a product (4 roundings) and the device log; then
    S1 + (Sy - Sx) on the host (2 roundings), each sum over its own tree"""
    from accbpg_and_fw_amd.functions import shannon_ls_terms
    h = data(n)
    d = h["d"]
    delta = 1e-20
    k = 4 + ulps[0] + 2
    depth = T.tree_depth(n, T.CAP_WIDE)
    lin, got_xy, got_zw = shannon_ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"], delta)
    for name, got, (ref, mag) in (("D(x,y)", got_xy, _shannon(h["px"], h["py"], delta)),
                                  ("D(z,w)", got_zw, _shannon(h["pz"], h["pw"], delta))):
        print("n %d depth %d %s err %.3e bound %.3e" % (n, depth, name, abs(got - ref), (depth + k) * EPS * mag))
        assert abs(got - ref) <= (depth + k) * EPS * mag
    assert acc.ShannonEntropy(delta).divergence(d["px"], d["py"]) == got_xy


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_shannon_simplex_prox_normaliser(acc, ulps, n):
    """x_i = exp(-g_i/L - 1) (or y_i exp(-g_i/L)), then x / sum x with the sum taken by block_total.  Elementwise
    relative error of x_i: the roundings of q = -g/L and q - 1 pass through exp as absolute errors of its argument,
    (|q| + |q - 1|) eps/2, then the device exp, then (div form) the product with y.  The normaliser adds
    tree_depth * eps and the same elementwise figure, the division one more rounding."""
    h = data(n)
    d = h["d"]
    hs = acc.ShannonEntropySimplex()
    L = 1.7
    q = -h["g"].astype(LD) / LD(L)
    depth = T.tree_depth(n, T.CAP_WIDE)
    for y in (None, "py"):
        got = (hs.prox_map(d["g"], L) if y is None else hs.div_prox_map(d[y], d["g"], L)).cpu().numpy()
        e = np.exp(q - 1) if y is None else h[y].astype(LD) * np.exp(q)
        ref = e / LD(fsum_ld(e))
        arg = float(np.max(np.abs(q) + (np.abs(q - 1) if y is None else 0)))
        elem = (arg / 2 + ulps[1] + (1 if y is not None else 0)) * EPS
        bound = 2 * elem + (depth + 1) * EPS
        err = float(np.max(np.abs(got.astype(LD) - ref) / ref))
        total = math.fsum(got)
        print("n %d depth %d y %s rel err %.3e bound %.3e |sum-1| %.3e" % (n, depth, y, err, bound, abs(total - 1)))
        assert err <= bound
        assert abs(total - 1) <= depth * EPS


# =================================================================================================== (e) NaN and sign
@pytest.mark.parametrize("n", VEC_SIZES)
def test_nan_zero_negative_through_the_vec_and_inexact_trees(acc, n):
    from accbpg_and_fw_amd.functions import combine_ls_terms, ls_terms, vec_min_sum
    cs = [torch.full((n,), 2.0 + i, dtype=torch.float64, device="cuda") for i in range(4)]
    g = data(n)["d"]["g"]
    gneg = -g.abs() - 0.5                                                 # every entry pays: the LMO asserts
    burg = acc.BurgEntropy()
    ls_terms(g, *cs)                                                      # positive data passes
    combine_ls_terms(burg, 0.5, cs[0], 0.5, cs[1], 1.0, g, cs[2])
    for j, p in enumerate(T.planted_positions(n, T.CAP_VEC)):
        for bad in (float("nan"), 0.0, -1.0):
            with planted(cs[0], p, bad):
                mn, sm = vec_min_sum(cs[0])
                assert (np.isnan(mn) and np.isnan(sm)) if bad != bad else (mn, sm) == (bad, 2.0 * (n - 1) + bad), (p, bad)
            with planted(cs[j % 4], p, bad):                              # x, y, z, z1 in turn
                with pytest.raises(AssertionError, match="not positive"):
                    ls_terms(g, *cs)
                if j % 4 < 2:
                    with pytest.raises(AssertionError, match="not positive"):
                        burg.divergence(cs[0], cs[1])
            with planted(cs[2], p, bad):                                  # the reference point
                with pytest.raises(AssertionError, match="not positive"):
                    combine_ls_terms(burg, 0.5, cs[0], 0.5, cs[1], 1.0, g, cs[2])
            with planted(cs[0], p, bad):                                  # the combined point w = (u + u)/2
                with pytest.raises(AssertionError, match="not positive"):
                    combine_ls_terms(burg, 0.5, cs[0], 0.5, cs[0], 1.0, g, cs[2])
        # a NaN centre makes min s a NaN: the epsilon assertion of the positive-orthant LMO fires
        with planted(cs[1], p, float("nan")):
            with pytest.raises(AssertionError, match="epsilon-nonnegativity"):
                acc.lmo_l2_ball_positive_orthant(1.0, center=cs[1], epsilon=1e-7)(gneg)
    acc.lmo_l2_ball_positive_orthant(1.0, center=cs[1], epsilon=1e-7)(gneg)


@pytest.mark.parametrize("n", WIDE_SIZES)
def test_nan_zero_negative_through_the_shannon_tree(acc, n):
    from accbpg_and_fw_amd.functions import shannon_ls_terms
    cs = [torch.full((n,), 2.0 + i, dtype=torch.float64, device="cuda") for i in range(4)]
    g = data(n)["d"]["g"]
    clean = shannon_ls_terms(g, *cs)
    for j, p in enumerate(T.planted_positions(n, T.CAP_WIDE)):
        with planted(cs[j % 4], p, 0.0):                                  # zeros are inside the domain
            assert np.all(np.isfinite(shannon_ls_terms(g, *cs))), p
        for bad in (float("nan"), -1.0, -1e-300):
            with planted(cs[j % 4], p, bad):
                with pytest.raises(AssertionError, match="negative"):
                    shannon_ls_terms(g, *cs)
                if j % 4 < 2:
                    with pytest.raises(AssertionError, match="negative"):
                        acc.ShannonEntropy().divergence(cs[0], cs[1])
    assert shannon_ls_terms(g, *cs) == clean


# =================================================================================================== (f) scratch
def test_interleaved_reductions_repeat_bit_for_bit(acc):
    """a 4-slot and two 8-slot reductions at a capped size, interleaved: all share ws + n of the size's workspace and
    the 16-double device scratch"""
    from accbpg_and_fw_amd.functions import ls_terms, quartic_ls_terms, shannon_ls_terms, vec_min_sum
    n = T.CAP_VEC * T.PER_BLOCK + 1
    d = data(n)["d"]
    calls = [lambda: ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"]),
             lambda: quartic_ls_terms(d["g"], d["x"], d["y"], d["z"], d["w"]),
             lambda: vec_min_sum(d["x"]),
             lambda: shannon_ls_terms(d["g"], d["px"], d["py"], d["pz"], d["pw"])]
    first = [c() for c in calls]
    for _ in range(10):
        for c, f in zip(calls, first):
            assert c() == f
    for _ in range(10):
        for c, f in zip(reversed(calls), reversed(first)):
            assert c() == f


@pytest.mark.parametrize("n", [T.PER_BLOCK, T.PER_BLOCK + 1, T.CAP_VEC * T.PER_BLOCK + 1])
def test_lmo_positive_orthant_two_passes_through_one_scratch(acc, n):
    h = data(n)
    d = h["d"]
    g, c = h["g"], h["py"]
    radius, eps = 0.7, 1e-7
    s, info = lmo_pos(d["g"], d["py"], radius, eps)
    neg = g < 0
    gnorm = np.sqrt(np.float64(T.tree_sum(np.where(neg, g * g, 0.0), T.CAP_VEC, single_block_final=False)))
    ref = np.maximum(c + radius * np.where(neg, -g / gnorm, 0.0), eps)
    sn = s.cpu().numpy()
    np.testing.assert_allclose(sn, ref, rtol=1e-15, atol=0)
    diff = sn - c
    assert info[0] == float(np.count_nonzero(neg)) == T.tree_sum(neg.astype(np.float64), T.CAP_VEC, False)
    assert info[1] == np.sqrt(np.float64(T.tree_sum(diff * diff, T.CAP_VEC, single_block_final=False)))
    assert info[2] == sn.min()
    got = acc.lmo_l2_ball_positive_orthant(radius, center=d["py"], epsilon=eps)(d["g"])
    assert torch.equal(got, s)
    s2, info2 = lmo_pos(d["g"], d["py"], radius, eps)
    assert torch.equal(s2, s) and info2 == info


# =================================================================================================== (g) batched ls_terms
def test_batched_ls_terms_equals_single_instances(acc):
    """K = 2 at n = 2**20 + 1, one entry past the cap: the design matrices behind the batch handle are never read by
    ls_terms, so two rows of zeros stand in for them (m = 2) and the batch is made at the full size."""
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import ls_terms
    lib = _lib.load()
    n = T.CAP_VEC * T.PER_BLOCK + 1
    K, m = 2, 2
    d = data(n)["d"]
    V = torch.zeros(m, n, dtype=torch.float64, device="cuda")
    G = torch.stack([d["g"], d["x"]])
    X = torch.stack([d["px"], d["pz"]])
    Y = torch.stack([d["py"], d["pw"]])
    Z = torch.stack([d["pz"], d["py"]])
    Z1 = torch.stack([d["pw"], d["px"]])
    hb = C.c_void_p()
    arr = (C.c_void_p * K)(V.data_ptr(), V.data_ptr())
    _lib.check(lib.accbpg_dopt_batch_create(arr, K, m, n, n, None, C.byref(hb)), "accbpg_dopt_batch_create")
    try:
        for active in (None, [1, 1], [0, 1], [1, 0]):
            out = (C.c_double * (3 * K))(*([-7.0] * (3 * K)))
            st = (C.c_int * K)(*([-1] * K))
            mask = (C.c_int * K)(*active) if active else None
            rc = lib.accbpg_dopt_batch_ls_terms(hb, G.data_ptr(), X.data_ptr(), Y.data_ptr(), Z.data_ptr(), Z1.data_ptr(),
                                                n, mask, out, st)
            assert rc == 0, _lib.last_error()
            for i in range(K):
                if active and not active[i]:
                    assert list(out[3 * i:3 * i + 3]) == [-7.0] * 3 and st[i] == -1
                else:
                    assert st[i] == 0
                    assert tuple(out[3 * i:3 * i + 3]) == ls_terms(G[i], X[i], Y[i], Z[i], Z1[i]), i
        with planted(Y[1], n - 1, 0.0):                                   # instance 1 alone fails its assertion
            out = (C.c_double * (3 * K))()
            st = (C.c_int * K)(-1, -1)
            assert lib.accbpg_dopt_batch_ls_terms(hb, G.data_ptr(), X.data_ptr(), Y.data_ptr(), None, None, n, None, out,
                                                  st) == 0
            assert list(st) == [0, _lib.ERR_ASSERT]
            assert tuple(out[0:2]) == ls_terms(G[0], X[0], Y[0])[:2]
    finally:
        lib.accbpg_dopt_batch_destroy(hb)
