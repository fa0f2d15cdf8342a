"""GPU tests of accbpg_fw_direction (vec_kernels.hip) through functions_lmo.fw_direction: the fused Frank-Wolfe
direction step against the composition it replaces.

For each of the three oracles (l2 ball, l-infinity ball, simplex) with the centre None, a scalar and an array, at the
sizes at which the reduction tree changes shape: s and d are bit-equal to lmo(g) followed by vec_axpby(1, s, -1, x);
sum g^2, <g, d> and sum d^2 are bit-equal to reduce_numpy.tree_sum over the once-rounded elementwise terms g*g, g*d and
d*d of the device's own d (and so to vec_dot on them); the vertex index is the first argmin under planted ties.  Then
||g|| on either side of 1e-10, a NaN in g, and the l2 ball's boundary assertion."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_numpy as T  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = sorted(set([1, 2, 63, 64, 65, 1025] + T.edge_sizes(T.CAP_VEC)))
KINDS = ("l2", "linf", "simplex")
CENTERS = ("none", "scalar", "array")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def bits(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).copy()
    a[np.isnan(a)] = np.nan
    return a.view(np.int64)


def same_bits(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def oracle(acc, kind, center, n, radius):
    c = {"none": None, "scalar": 0.25, "array": T.draw(n, 11) * 0.5}[center]
    if kind == "l2":
        return acc.lmo_l2_ball(radius, c)
    if kind == "linf":
        return acc.lmo_linf_ball(radius, c)
    return acc.lmo_simplex(radius)


def check(acc, lmo, g, x):
    """fw_direction against the composition and the emulated tree -> (s, d, gg, slope, dd, idx, dist)"""
    gd, xd = torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda()
    out = acc.fw_direction(lmo, gd, xd)
    s, d, gg, slope, dd, idx, dist = out
    s_ref = lmo(gd).reshape(-1)
    d_ref = acc.functions.vec_axpby(1.0, s_ref, -1.0, xd)
    sh, dh = s.cpu().numpy(), d.cpu().numpy()
    assert same_bits(sh, s_ref.cpu().numpy()) and same_bits(dh, d_ref.cpu().numpy())
    with np.errstate(all="ignore"):
        assert same_bits(gg, T.tree_sum(g * g, T.CAP_VEC))
        assert same_bits(slope, T.tree_sum(g * dh, T.CAP_VEC))
        assert same_bits(dd, T.tree_sum(dh * dh, T.CAP_VEC))
    assert same_bits(gg, acc.functions.vec_dot(gd, gd)) and same_bits(slope, acc.functions.vec_dot(gd, d_ref))
    assert same_bits(dd, acc.functions.vec_dot(d_ref, d_ref))
    assert same_bits(dd * 0.5, acc.SquaredL2Norm().divergence(s_ref, xd))
    return out


@pytest.mark.parametrize("n", SIZES)
def test_direction_is_the_composition_bit_for_bit(acc, n):
    g, x = T.draw(n, 21), T.draw(n, 22) * 0.3
    for kind in KINDS:
        for center in (CENTERS if kind != "simplex" else CENTERS[:1]):      # (the simplex has no centre)
            lmo = oracle(acc, kind, center, n, 1.5)
            assert (lmo.kind, lmo.radius) == (KINDS.index(kind), 1.5)
            s, d, gg, slope, dd, idx, dist = check(acc, lmo, g, x)
            if kind == "simplex":
                assert idx == int(np.argmin(g)) and s[idx].item() == 1.5
            if kind == "l2":
                assert abs(dist - 1.5) <= 1e-10


@pytest.mark.parametrize("n", [1, 65, 1025, 4097, 262145])
def test_vertex_is_the_first_argmin_under_ties(acc, n):
    g = np.abs(T.draw(n, 5)) + 1.0
    for p in T.planted_positions(n, T.CAP_VEC)[::-1]:
        g[p] = -2.0                                             # ties, planted from the back: the first one must win
        x = np.full(n, 1.0 / n)
        _, _, _, _, _, idx, _ = check(acc, acc.lmo_simplex(), g, x)
        assert idx == int(np.argmin(g)) == p


def test_l2_ball_on_either_side_of_the_small_norm(acc):
    n = 1025
    u = T.draw(n, 3)
    u /= np.linalg.norm(u)
    x = T.draw(n, 4)
    c = T.draw(n, 6)
    for center in (None, 0.5, c):
        lmo = acc.lmo_l2_ball(2.0, center)
        for scale, centre in ((0.5e-10, True), (0.999e-10, True), (1.001e-10, False), (4e-10, False)):
            g = u * scale
            s, d, gg, slope, dd, idx, dist = check(acc, lmo, g, x)
            assert (np.sqrt(gg) < 1e-10) == centre
            cfull = np.broadcast_to(0.0 if center is None else center, (n,))
            assert same_bits(s.cpu().numpy(), cfull) == centre
            assert (dist == 0.0) == centre
    # a zero gradient: the centre, slope 0
    s, d, gg, slope, dd, idx, dist = check(acc, acc.lmo_l2_ball(2.0, c), np.zeros(n), x)
    assert gg == 0.0 and slope == 0.0 and same_bits(s.cpu().numpy(), c)


def test_nan_in_g(acc):
    n = 1025
    g, x = T.draw(n, 8), T.draw(n, 9)
    g[700] = np.nan
    gd, xd = torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda()
    # the simplex: np.argmin takes the first NaN; the sums are NaN
    s, d, gg, slope, dd, idx, dist = check(acc, acc.lmo_simplex(), g, x)
    assert idx == 700 and np.isnan(gg) and np.isnan(slope) and np.isfinite(dd)
    # the l-infinity ball: sign(NaN) = NaN in that entry only
    s, d, gg, slope, dd, idx, dist = check(acc, acc.lmo_linf_ball(1.0), g, x)
    assert np.isnan(s.cpu().numpy()).sum() == 1 and np.isnan(dd)
    # the l2 ball: the norm is NaN, every entry is, and the boundary assertion fails as in lmo_l2_ball itself
    with pytest.raises(AssertionError, match="ball boundary"):
        acc.lmo_l2_ball(1.0)(gd)
    with pytest.raises(AssertionError, match="ball boundary"):
        acc.fw_direction(acc.lmo_l2_ball(1.0), gd, xd)


def test_boundary_assertion_and_arguments(acc):
    """a centre of 1e10 swallows the step's low bits: ||(c - t) - c|| misses the radius by more than 1e-10"""
    n = 65
    g, x = T.draw(n, 1), T.draw(n, 2)
    gd, xd = torch.from_numpy(g).cuda(), torch.from_numpy(x).cuda()
    lmo = acc.lmo_l2_ball(1.0, 1e10)
    with pytest.raises(AssertionError, match="ball boundary"):
        lmo(gd)
    with pytest.raises(AssertionError, match="ball boundary"):
        acc.fw_direction(lmo, gd, xd)
    with pytest.raises(AssertionError):
        acc.fw_direction(lambda v: v, gd, xd)                   # not an oracle of the package
    with pytest.raises(AssertionError):
        acc.fw_direction(acc.lmo_simplex(), gd, xd[:-1])
    # an n x r iterate goes through flat and comes back in its shape
    G, X = torch.from_numpy(T.draw(12, 3).reshape(4, 3)).cuda(), torch.from_numpy(T.draw(12, 4).reshape(4, 3)).cuda()
    lmo = acc.lmo_linf_ball(0.5, T.draw(12, 5).reshape(4, 3))
    s, d = acc.fw_direction(lmo, G, X)[:2]
    assert s.shape == (4, 3) and same_bits(s.cpu().numpy(), lmo(G).cpu().numpy())
    assert same_bits(d.cpu().numpy(), (lmo(G) - X).cpu().numpy())
