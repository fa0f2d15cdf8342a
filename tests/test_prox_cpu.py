"""Host-side validation of tests/prox_numpy.py, the restatement and bounds that tests/test_gpu_prox.py holds the Burg
simplex prox kernels to: the bounds are shown on the reference alone (a float64 replay against the long double one),
the condition under which Newton counts are compared holds for every case, and the restatement is the oracle's loop."""
import numpy as np
import pytest

import prox_numpy as P
from oracle import np_oracle


def _replays(n, fam, L, eps, form):
    y, g = P.inputs(n, fam, L, form)
    gg = P.make_gg(y, g, L)
    return gg, P.replay(gg, eps, np.longdouble), P.replay(gg, eps, np.float64)


def _validate(variant, n, eps, gg, R, R64):
    lv = P.launched(variant, n)
    assert abs(gg.min()) <= 2.0 ** 40                     # cmin + 1 does not round: phi(cmin + 1) >= 0, no bisection
    assert R.nb == 0 and R64.nb == 0
    if not P.stall_regime(R, eps):
        assert P.count_margin_ok(R, eps, lv, n)
        assert (R64.nb, R64.nn) == (R.nb, R.nn) and not R64.stalled
    assert abs(float(np.longdouble(R64.c[-1]) - R.c[-1])) <= 0.25 * P.c_bound(R, lv, n)
    f, S, d = P.phi_at(gg, float(R64.c[-1]))
    if P.stall_regime(R, eps):
        assert abs(float(f)) <= P.phi_err(lv, n, S) + P.c_quantum(R64.c[-1], d)
    else:
        assert abs(float(f)) <= eps + P.phi_err(lv, n, S)


@pytest.mark.parametrize("fam,L,eps", P.DATA)
def test_bounds_hold_for_the_float64_replay_on_every_case(fam, L, eps):
    """For every case of the GPU module: no bisection; outside the stall regime the margin condition of the count
    comparison holds and the float64 replay takes the reference's counts; its c lies within a quarter of the bound of
    (c) of the reference's; its phi meets (b).  np.sum adds pairwise, a shallower tree than any kernel's, so this
    shows the bounds on the reference alone and says nothing about a kernel."""
    stalls = 0
    for form in ("div", "prox"):
        for n in sorted({n for _, n in P.FORCED + P.PRODUCTION}):
            gg, R, R64 = _replays(n, fam, L, eps, form)
            stalls += P.stall_regime(R, eps)
            for variant in sorted({v for v, m in P.FORCED + P.PRODUCTION if m == n}):
                _validate(variant, n, eps, gg, R, R64)
    # the vertex family is where a float64 step of c is coarser than eps; nowhere else do the cases stall
    assert (stalls > 0) == (fam == "vertex")


@pytest.mark.parametrize("n,expect", P.THRESHOLDS)
def test_threshold_inputs_meet_the_margin_condition(n, expect):
    """the six sizes of test_production_thresholds, the two largest included (where the GPU test compares with the
    float64 replay and relies on the quarter shown here)"""
    assert P.by_size(n) == expect
    gg, R, R64 = _replays(n, "random", 1.0, 1e-8, "div")
    assert not P.stall_regime(R, 1e-8)
    _validate(0, n, 1e-8, gg, R, R64)


def test_dispatch_table():
    assert [P.by_size(n) for n in (1, 2048, 2049, 8192, 8193, 32768, 32769, 1048576, 1048577, 4194304, 4194305)] \
        == [10, 10, 11, 11, 12, 12, 2, 2, 3, 3, 1]
    assert P.workgroups(2, 8193) == 2 and P.workgroups(2, 3 * 8192) == 3 and P.workgroups(3, 32769) == 2
    assert P.workgroups(2, 1048576) == 128 and P.workgroups(3, 4194304) == 128 and P.workgroups(3, 4194305) == 129
    assert P.depth(1, 4194305) == 4097 + 22 and P.depth(12, 32768) == 32 + 22 and P.depth(3, 4194304) == 32 + 22 + 128


@pytest.mark.parametrize("n", [1, 2, 65, 2049, 8193])
def test_float64_replay_is_the_oracle(n):
    """the same loop as oracle.np_oracle.BurgSimplexOracle (left-to-right sums there, pairwise here): equal counts,
    x to 1e-13"""
    ho = np_oracle.BurgSimplexOracle()
    for L in (1.0, 0.02):
        y, g = P.random_family(n, n)
        xo = ho.div_prox_map(y, g, L)
        R = P.replay(P.make_gg(y, g, L), 1e-8, np.float64)
        assert (R.nb, R.nn) == (ho.last_bisect_steps, ho.last_newton_steps)
        np.testing.assert_allclose(R.x, xo, rtol=1e-13, atol=0)
        xo = ho.prox_map(g, L)
        R = P.replay(P.make_gg(None, g, L), 1e-8, np.float64)
        assert (R.nb, R.nn) == (ho.last_bisect_steps, ho.last_newton_steps)
        np.testing.assert_allclose(R.x, xo, rtol=1e-13, atol=0)


def test_make_gg_is_the_oracle_argument():
    y, g = P.random_family(777, 3)
    ho = np_oracle.BurgSimplexOracle()
    for L in (1.0, 0.02):
        np.testing.assert_array_equal(P.make_gg(y, g, L), (g - L * ho.gradient(y)) / L)
        np.testing.assert_array_equal(P.make_gg(None, g, L), g / L)


@pytest.mark.parametrize("n", [1, 65, 5000, 40000])
def test_recover_c(n):
    """finds the c of a NumPy-made output; refuses one entry moved by one ulp, a dropped and a swapped entry"""
    for fam in ("random", "vertex", "mixed"):
        y, g = P.inputs(n, fam, 1.0, "div")
        gg = P.make_gg(y, g, 1.0)
        R = P.replay(gg, 1e-8, np.float64)
        c = P.recover_c(gg, R.x, near=R.c[-1])
        np.testing.assert_array_equal(1.0 / (gg + c), R.x)
        assert abs(c - float(R.c[-1])) <= 2 * np.spacing(abs(float(R.c[-1])))
        for k in sorted({0, n // 2, n - 1}):
            x = R.x.copy()
            x[k] = np.nextafter(x[k], 0.0)
            with pytest.raises(ValueError):
                P.recover_c(gg, x)
        if n > 1:
            x = R.x.copy()
            x[n - 1] = x[n - 2]                           # the tail entry duplicated from its neighbour
            with pytest.raises(ValueError):
                P.recover_c(gg, x)


def test_replay_of_a_nan_argument():
    gg = P.make_gg(None, np.array([-3.0, -1.0, np.nan]), 1.0)
    for dt in (np.float64, np.longdouble):
        R = P.replay(gg, 1e-8, dt)
        assert (R.nb, R.nn) == (0, 0) and np.all(np.isnan(R.x))
