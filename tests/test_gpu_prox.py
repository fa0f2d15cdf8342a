"""Every launch form of the Burg simplex prox (accbpg_burg_simplex_div_prox), thresholds included, against the long
double replay of tests/prox_numpy.py on the kernel's own gg.

What a case asserts (prox_numpy has the bounds and where their constants come from):
 (a) form      one float64 c reproduces every output entry bit for bit as 1/(gg_i + c)  (recover_c);
 (b) stop      |phi(c)| <= eps + phi_err, phi in long double at that c; in the stall regime (one float64 step of c
               moves phi by eps or more, or the reference left by the stall test) <= phi_err + u |c| |phi'|;
 (c) iterate   the (bisection, Newton) counts of the long double replay, bisection 0, and
               |c - c_R| <= 8 (phi_err / |phi'_R| + u |c_R|); in the stall regime the stopping decision is a rounding
               matter and only c is compared;
 (d) launch    accbpg_debug_prox_state names the expected kernel and workgroup count, and the "multi off" latch is 0.
tests/test_prox_cpu.py shows on the host that every case meets the margin condition of the count comparison and that
the bound of (c) holds for a float64 replay with room to spare.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

import prox_numpy as P

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def lib(acc):
    from accbpg_and_fw_amd import _lib
    return _lib.load()


@contextlib.contextmanager
def forced(lib, variant):
    assert lib.accbpg_debug_prox_variant(variant) == 0
    try:
        yield
    finally:
        lib.accbpg_debug_prox_variant(0)


def state(lib):
    out = (C.c_int * 3)(-1, -1, -1)
    assert lib.accbpg_debug_prox_state(out) == 0
    return out[0], out[1], out[2]


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(acc, lib, variant, y, g, L, eps):
    """one prox call under the switch -> (x on the host, (bisection, Newton), state)"""
    h = acc.BurgEntropySimplex(eps)
    with forced(lib, variant):
        x = h.prox_map(dev(g), L) if y is None else h.div_prox_map(dev(y), dev(g), L)
        st = state(lib)
    return x.cpu().numpy(), tuple(h.last_info), st


def check(variant, n, gg, eps, x, info, st, R, c_slack=1.0):
    """(a) - (d) of the module docstring; R is the reference replay on gg"""
    lv = P.launched(variant, n)
    assert st == (lv, P.workgroups(lv, n), 0), st                                     # (d)
    c = P.recover_c(gg, x, near=R.c[-1])                                              # (a)
    f, S, d = P.phi_at(gg, c)
    perr = P.phi_err(lv, n, S)
    stall = P.stall_regime(R, eps)
    print("variant %d n %d: counts %s ref (%d, %d) stall %d |phi| %.3e phi_err %.3e |c - c_R| %.3e bound %.3e"
          % (lv, n, info, R.nb, R.nn, stall, abs(float(f)), perr, abs(float(np.longdouble(c) - R.c[-1])),
             c_slack * P.c_bound(R, lv, n)))
    if stall:                                                                         # (b)
        assert abs(float(f)) <= perr + P.c_quantum(c, d)
    else:
        assert abs(float(f)) <= eps + perr
    assert R.nb == 0 and info[0] == 0                                                 # (c)
    if not stall:
        assert P.count_margin_ok(R, eps, lv, n)          # a condition on the input (test_prox_cpu.py), not on the kernel
        assert info == (R.nb, R.nn)
    assert abs(float(np.longdouble(c) - R.c[-1])) <= c_slack * P.c_bound(R, lv, n)
    return c


# ------------------------------------------------------------------ every form on every data family
@pytest.mark.parametrize("case", P.CASES, ids=P.case_id)
def test_prox_case(acc, lib, case):
    variant, n, fam, L, eps, form = case
    y, g = P.inputs(n, fam, L, form)
    gg = P.make_gg(y, g, L)
    x, info, st = run(acc, lib, variant, y, g, L, eps)
    check(variant, n, gg, eps, x, info, st, P.replay(gg, eps, np.longdouble))
    if fam == "equal":                                   # a tie of all entries: every entry the same double
        assert np.all(x == x[0])


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("n", [1025, 5000, 32768])
def test_reread_form_equals_register_form_bit_for_bit(acc, lib, n):
    """burg_prox_kernel<0> and the register form the size selects add the same entries in the same order: thread t
    owns t, t + 1024, ... in both, and the wave and workgroup stages are the same code."""
    for L in (1.0, 0.02):
        for form in ("div", "prox"):
            y, g = P.inputs(n, "random", L, form)
            x0, i0, s0 = run(acc, lib, 0, y, g, L, 1e-8)
            x1, i1, s1 = run(acc, lib, 1, y, g, L, 1e-8)
            assert s0[0] == P.by_size(n) and s1[0] == 1
            assert i0 == i1
            np.testing.assert_array_equal(x0.view(np.int64), x1.view(np.int64))


@pytest.mark.parametrize("multi,n", [(2, 8193), (2, 40000), (3, 32769), (3, 5 * 32768)])
def test_multi_forms_against_one_workgroup(acc, lib, multi, n):
    """Another order of summation, the same iteration: equal counts and a c within the bound of (c) (the larger of
    the two forms') of the one-workgroup result."""
    for L in (1.0, 0.02):
        y, g = P.inputs(n, "random", L, "div")
        gg = P.make_gg(y, g, L)
        R = P.replay(gg, 1e-8, np.longdouble)
        xm, im, sm = run(acc, lib, multi, y, g, L, 1e-8)
        x1, i1, s1 = run(acc, lib, 1, y, g, L, 1e-8)
        assert sm[:2] == (multi, P.workgroups(multi, n)) and s1[:2] == (1, 1) and sm[2] == 0 and s1[2] == 0
        assert im == i1
        cm, c1 = P.recover_c(gg, xm, near=R.c[-1]), P.recover_c(gg, x1, near=R.c[-1])
        assert abs(cm - c1) <= max(P.c_bound(R, multi, n), P.c_bound(R, 1, n))


# ------------------------------------------------------------------ thresholds of the production dispatch
@pytest.mark.parametrize("n,expect", P.THRESHOLDS)
def test_production_thresholds(acc, lib, n, expect):
    """Either side of 32768, 1048576 and 4194304 under production dispatch: 12, 2, 2, 3, 3, 1.  (a), (b), (d) as
    everywhere.  (c) against the long double replay up to n = 1048577; at the two largest sizes that replay alone takes
    seconds, so (c) is taken from the float64 replay there, with a quarter more room: test_prox_cpu.py shows the
    float64 replay within a quarter of the bound of the long double one at these very inputs."""
    assert P.by_size(n) == expect
    y, g = P.inputs(n, "random", 1.0, "div")
    gg = P.make_gg(y, g, 1.0)
    x, info, st = run(acc, lib, 0, y, g, 1.0, 1e-8)
    assert st[0] == expect
    if n <= 1048577:
        check(0, n, gg, 1e-8, x, info, st, P.replay(gg, 1e-8, np.longdouble))
    else:
        check(0, n, gg, 1e-8, x, info, st, P.replay(gg, 1e-8, np.float64), c_slack=1.25)


# ------------------------------------------------------------------ edges
EDGE_N = 40000
EDGE_VARIANTS = [1, 2, 3, 0]


@pytest.mark.parametrize("variant", EDGE_VARIANTS)
@pytest.mark.parametrize("where,value", [("last", 0.0), ("first", -1.0)])
def test_nonpositive_y_is_refused(acc, lib, variant, where, value):
    """y[n-1] = 0 and y[0] = -1: the reference's assertion (functions.py:270); the next call on good data is right,
    bit for bit what it was before, and the latch stays 0."""
    n = EDGE_N
    y, g = P.inputs(n, "random", 1.0, "div")
    gg = P.make_gg(y, g, 1.0)
    x0, i0, s0 = run(acc, lib, variant, y, g, 1.0, 1e-8)
    yb = y.copy()
    yb[n - 1 if where == "last" else 0] = value
    h = acc.BurgEntropySimplex(1e-8)
    with forced(lib, variant):
        with pytest.raises(AssertionError, match=P.MSG):
            h.div_prox_map(dev(yb), dev(g), 1.0)
        assert state(lib) == (P.launched(variant, n), P.workgroups(P.launched(variant, n), n), 0)
    x1, i1, s1 = run(acc, lib, variant, y, g, 1.0, 1e-8)
    check(variant, n, gg, 1e-8, x1, i1, s1, P.replay(gg, 1e-8, np.longdouble))
    assert i1 == i0 and s1 == s0
    np.testing.assert_array_equal(x1.view(np.int64), x0.view(np.int64))


def test_forced_multi_form_with_too_many_workgroups(acc, lib):
    """more than 128 workgroups: ValueError, nothing launched (the state still describes the call before)"""
    y, g = P.inputs(1025, "random", 1.0, "div")
    run(acc, lib, 1, y, g, 1.0, 1e-8)
    for variant, n in [(2, 128 * 8192 + 1), (3, 128 * 32768 + 1)]:
        before = state(lib)
        gd = torch.full((n,), -2.0, dtype=torch.float64, device="cuda")
        gg = np.full(n - 1, -2.0)
        with forced(lib, variant):
            with pytest.raises(ValueError):
                acc.BurgEntropySimplex().prox_map(gd, 1.0)
            assert state(lib) == before
            h = acc.BurgEntropySimplex()                  # one entry fewer: 128 workgroups, runs
            x = h.prox_map(gd[:-1], 1.0)
            assert state(lib) == (variant, 128, 0)
        x = x.cpu().numpy()
        assert np.all(x == x[0])
        f, S, d = P.phi_at(gg, P.recover_c(gg, x))
        assert abs(float(f)) <= 1e-8 + P.phi_err(variant, n - 1, S)


@pytest.mark.parametrize("variant", EDGE_VARIANTS)
def test_nan_argument_gives_nan_everywhere(acc, lib, variant):
    """g[n-1] = NaN: np.min keeps it, every comparison of functions.py:345-349 is False, so the reference returns an
    all-NaN vector after (0, 0) steps -- and so does every form, without an error and without tripping the latch (all
    workgroups see bit-identical totals and leave together)."""
    n = EDGE_N
    for form in ("div", "prox"):
        y, g = P.inputs(n, "random", 1.0, form)
        g = g.copy()
        g[n - 1] = np.nan
        R = P.replay(P.make_gg(y, g, 1.0), 1e-8, np.float64)
        assert (R.nb, R.nn) == (0, 0) and np.all(np.isnan(R.x))
        x, info, st = run(acc, lib, variant, y, g, 1.0, 1e-8)
        assert np.all(np.isnan(x)) and x.shape == (n,)
        assert info == (0, 0)
        assert st == (P.launched(variant, n), P.workgroups(P.launched(variant, n), n), 0)


# ------------------------------------------------------------------ the latch, last
def test_latch_stays_clear_beside_the_overlapped_value_evaluation(acc, lib):
    """ABPG_gain with the value evaluation on the side stream at n just above 32768: the multi-workgroup prox runs
    beside another stream's one-launch Cholesky.  It must not have given up a wait."""
    m, n = 256, 33024
    assert state(lib)[2] == 0
    f, h, L, x0 = acc.D_opt_design(m, n, randseed=5)
    f.overlap_values(True)
    acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=20, verbose=False)
    assert state(lib) == (2, P.workgroups(2, n), 0)
