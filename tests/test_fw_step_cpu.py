"""The one-step NumPy restatement of the Frank-Wolfe solvers (tests/fw_numpy.py) against the oracle, without a GPU:
chained with the solvers' own decision code (``_fw_decide`` / ``_AwayRun.iterate``) it reproduces ``np_oracle.D_opt_FW``
and ``D_opt_FW_away`` -- bit for bit on axis designs, at the bars of test_gpu_parity.test_fw_trajectories on Gaussian
ones -- and the exactness preconditions of the axis designs hold in rational arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import fw_numpy as N
from conftest import gaussian_design
from oracle import np_oracle as O


def _decide():
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    return _fw_decide, (lambda m, maxitrs: _AwayRun(m, maxitrs, 0, 1))


def _axis(m, n, start):
    s, x0 = N.axis_run_design(m, n, start)
    V, G = N.axis_design(m, n, s, x0)
    return s, x0, V, G


# ------------------------------------------------------------------------------------------------ probe / update
def test_probe_is_the_reference_expression():
    rng = np.random.RandomState(5)
    w = rng.rand(50) + 1.0
    x = rng.rand(50) * (rng.rand(50) > 0.5)
    w[7] = w[31] = w.max() + 1.0                      # tied maxima
    x[11] = x[40] = 0.3
    w[11] = w[40] = 0.5                               # tied supported minima
    i = np.argmax(w)
    sup = w[x > 0]
    assert N.probe(w, x, 0)[:2] == (7, 11)
    assert N.probe(w, x, 0).w_j == sup[np.argmin(sup)]
    assert N.probe(w, x, 1) == (7, int(np.argmin((w - w[i]) * [x > 1.0e-8])), w[7], 0.5, 0.3)
    x[11] = 1.0e-8                                    # inside the Frank-Wolfe support, outside the away support
    assert N.probe(w, x, 0).j == 11 and N.probe(w, x, 1).j == 40
    w[20] = np.nan                                    # NumPy: the first NaN is both extrema
    x[20] = 0.1
    assert N.probe(w, x, 0)[:2] == (20, 20) and N.probe(w, x, 1)[:2] == (20, 0)


def test_update_ref_agrees_with_float64():
    V = gaussian_design(37, 203, 3)
    x, det, H, w = N.setup_f64(V, np.ones(203) / 203)
    Hn, wn = N.update_f64(V, H, w, 17, -0.3, 0.9)
    ref = N.update_ref(V, H, w, 17, -0.3, 0.9)
    assert np.max(np.abs(Hn - ref.H) / (np.abs(H) + 0.3 * np.outer(ref.A, ref.A))) < N.gamma(2 * 37 + 5)
    assert np.max(np.abs(wn - ref.w) / (np.abs(w) + 0.3 * ref.B ** 2)) < N.gamma(4 * 37 + 5)
    assert np.all(np.abs(ref.Hv) <= ref.A) and np.all(ref.C <= ref.B) and abs(ref.q) <= ref.Q
    x2 = N.update_x(x, 5, 0.7, -0.01)
    assert x2[5] == x[5] * 0.7 + -0.01 and x2[6] == x[6] * 0.7


# ------------------------------------------------------------------------------------------------- whole chains
@pytest.mark.parametrize("m,n,start", N.RUN_SHAPES)
def test_chain_is_the_oracle_bit_for_bit_on_axis_designs(m, n, start):
    fw_decide, make_run = _decide()
    s, x0, V, G = _axis(m, n, start)
    for eps in (-1.0, 1.0):
        xo, Fo, SPo, SNo, _ = O.D_opt_FW(V, x0, eps, 60)
        x, F, SP, SN, picks, state = N.run_fw(V, x0, eps, 60, fw_decide)
        for a, b in ((x, xo), (SP, SPo), (SN, SNo), (F, Fo)):
            np.testing.assert_array_equal(a, b)
        xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, eps, 60)
        x, F, SP, SN, picks, state = N.run_away(V, x0, eps, 60, make_run)
        for a, b in ((x, xo), (SP, SPo), (SN, SNo)):
            np.testing.assert_array_equal(a, b)
        assert np.all(np.isfinite(F)) and np.max(np.abs(F - Fo)) <= 1e-12 * (1 + np.max(np.abs(Fo)))
        assert len(F) == 60 or eps > 0
        if eps > 0:
            assert 2 < len(F) < 60                     # the run with eps = 1 stops by its test


@pytest.mark.parametrize("m,n,start", N.RUN_SHAPES)
def test_run_designs_take_both_kinds_of_step(m, n, start):
    fw_decide, make_run = _decide()
    s, x0, V, G = _axis(m, n, start)
    x, F, SP, SN, picks, (xs, ws, Hs) = N.run_away(V, x0, -1.0, 60, make_run)
    kinds = SP >= SN
    assert kinds.sum() >= 5 and (~kinds).sum() >= 5
    assert ws[xs > 0].min() > 1.0
    assert len(set(i for i, j in picks)) >= 4
    assert np.count_nonzero(Hs - np.diag(np.diag(Hs))) == 0      # H stays diagonal
    if n > 4096:
        assert min(i for i, j in picks) > n // 2                 # maxima beyond every low seam


@pytest.mark.parametrize("m,n,seed", [(8, 40, 11), (37, 203, 12)])
def test_chain_follows_the_oracle_on_gaussian_designs(m, n, seed):
    """bars of test_gpu_parity.test_fw_trajectories"""
    fw_decide, make_run = _decide()
    V = gaussian_design(m, n, seed)
    x0 = np.ones(n) / n
    xo, Fo, SPo, SNo, _ = O.D_opt_FW(V, x0, 1e-6, 200)
    x, F, SP, SN, picks, state = N.run_fw(V, x0, 1e-6, 200, fw_decide)
    assert len(F) == len(Fo) and np.max(np.abs(x - xo)) < 1e-9
    for a, b in ((F, Fo), (SP, SPo), (SN, SNo)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9)
    xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, 1e-6, 200)
    x, F, SP, SN, picks, state = N.run_away(V, x0, 1e-6, 200, make_run)
    assert abs(len(F) - len(Fo)) <= 2
    k = min(len(F), len(Fo))
    assert np.max(np.abs(x - xo)) < 1e-8
    np.testing.assert_allclose(F[:k], Fo[:k], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(SP[:k], SPo[:k], rtol=1e-8, atol=1e-8)


# ------------------------------------------------------------------------------------- exactness preconditions
@pytest.mark.parametrize("m,n,start,kind", [s + ("run",) for s in N.RUN_SHAPES] +
                         [(8, 40, 8, "base"), (8, 203, 100, "base"), (16, 4097, 1024, "base")])
def test_axis_preconditions_hold(m, n, start, kind):
    s, x0 = N.axis_run_design(m, n, start) if kind == "run" else N.axis_base(m, n, start)
    G = N.axis_exact(m, s, x0)
    V, Gd = N.axis_design(m, n, s, x0)
    assert list(Gd) == G
    np.testing.assert_array_equal(np.dot(V * x0, V.T), np.diag(G))
    x, det, H, w = N.setup_f64(V, x0)
    np.testing.assert_array_equal(H, np.diag(1.0 / np.array(G)))
    np.testing.assert_array_equal(w, s * s / np.array(G)[np.arange(n) % m])


def test_axis_preconditions_are_checked():
    m, n = 8, 40
    s, x0 = N.axis_base(m, n, 0)
    N.axis_exact(m, s, x0)
    bad = x0.copy(); bad[0] *= 2                       # G_00 = 5/64
    with pytest.raises(AssertionError):
        N.axis_exact(m, s, bad)
    bad = x0.copy(); bad[[0, 8, 16, 24]] *= 2          # G_00 = 1/8: a power of two, but an odd one
    with pytest.raises(AssertionError):
        N.axis_exact(m, s, bad)
    bad = s.copy(); bad[35] = 1.0 + 2.0 ** -30         # square not representable
    with pytest.raises(AssertionError):
        N.axis_exact(m, bad, x0)
    ok = s.copy(); ok[35] = 1.0 + 2.0 ** -20           # square exact: 1 + 2^-19 + 2^-40
    N.axis_exact(m, ok, x0)
    bad = x0.copy(); bad[0:8] = 0.0; bad[8:16] = 0.0; bad[16:24] = 0; bad[24:32] = 0
    with pytest.raises(AssertionError):
        N.axis_exact(m, s, bad)
