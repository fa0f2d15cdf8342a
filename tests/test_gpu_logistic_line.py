"""GPU tests of the margins LogisticRegression carries along a segment (logistic_kernels.hip): line_begin, line_value,
line_accept and func_grad_carried.

Exact data (tests/logistic_numpy.py: A integers, x multiples of 1/64, y = +-1) with an integer direction d and a step
that is a power of two: x + a d and A (x + a d) = A x + a (A d) are exact in float64 in any order, so the carried margin
fma(a, (A d)_i, (A x)_i) is the margin a fresh func_grad(x + a d) computes, and everything behind it must agree bit for
bit: line_value with func_grad(., 0), and after line_accept fitted(), losses(), weights() and func_grad_carried with a
fresh func_grad.  The shapes are EXACT_SHAPES -- both launch forms of the A x pass, odd n, n = 1, 2050 rows -- and two
with an odd lda, where the loads are scalar.

General data.  The carried margin of row i is off by at most
    |ds_i| <= gamma(device_chain(n) + 2) * (|A||x| + |a||A||d|)_i
(the chain of A x, the chain of A d scaled by |a|, the fma's rounding and that of y*z), softplus is 1-Lipschitz, and the
epilogue adds T_ULP ulps of t_i: the value lies within (1/m) sum_i (|ds_i| + ulps(T_ULP, t_i)) of the np.longdouble
value at the np.longdouble point.  After k carried accepts the margins are off by at most the sum of the k step bounds;
checked at k = 63, the last carried iteration of the default refresh = 64."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_numpy as LN  # noqa: E402

pytestmark = pytest.mark.gpu
LD = LN.LD


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def same_bits(a, b):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).copy()
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64)).copy()
    a[np.isnan(a)], b[np.isnan(b)] = np.nan, np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def padded(A, pad):
    """A in a (m, n + pad) device matrix whose gap columns hold NaN"""
    m, n = A.shape
    big = torch.full((m, n + pad), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :n] = torch.from_numpy(A)
    return big[:, :n]


def rows(f):
    return f.fitted(), f.losses(), f.weights()


def exact_line(acc, A, x, y, d, steps, pad=0):
    """the four entries against fresh evaluations at x + a d, bit for bit"""
    m, n = A.shape
    f = acc.LogisticRegression(padded(A, pad), torch.from_numpy(y).cuda())
    fresh = acc.LogisticRegression(A, y)
    xd, dd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    v0, g0 = f.func_grad(xd, 2)
    vc, gc = f.func_grad_carried(2)                             # at x itself: the value and the gradient again
    assert same_bits(vc, v0) and same_bits(gc.cpu().numpy(), g0.cpu().numpy())
    assert same_bits(f.func_grad_carried(0), v0) and same_bits(f.func_grad_carried(1).cpu().numpy(), g0.cpu().numpy())
    before = rows(f)
    f.line_begin(dd)
    for a in steps:
        xa = x + a * d
        assert np.array_equal((xa - x) / a, d)                  # the point is exact
        assert same_bits(f.line_value(a), fresh.func_grad(xa, 0))
        assert all(same_bits(p, q) for p, q in zip(rows(f), before))       # a trial leaves the rows alone
    a = steps[-1]
    f.line_accept(a)
    vf, gf = fresh.func_grad(x + a * d, 2)
    assert all(same_bits(p, q) for p, q in zip(rows(f), rows(fresh)))
    vc, gc = f.func_grad_carried(2)
    assert same_bits(vc, vf) and same_bits(gc.cpu().numpy(), gf)
    assert same_bits(f.func_grad_carried(0), vf) and same_bits(f.func_grad_carried(1, as_numpy=True), gf)
    return f


CASES = [(m, n, 0) for m, n in LN.EXACT_SHAPES] + [(7, 129, 3), (33, 4096, 5)]


@pytest.mark.parametrize("m,n,pad", CASES)
def test_exact_data_bit_for_bit(acc, m, n, pad):
    A, x, y = LN.exact_data(m, n, 100 * m + n)
    d = np.random.RandomState(m + n).randint(-3, 4, size=n).astype(np.float64)
    f = exact_line(acc, A, x, y, d, (1.0, 0.25, 2.0, 0.5), pad)
    # a second segment from the accepted point: the carried rows are a starting point like any other
    x1 = x + 0.5 * d
    d2 = np.random.RandomState(m + n + 1).randint(-3, 4, size=n).astype(np.float64)
    fresh = acc.LogisticRegression(A, y)
    f.line_begin(d2)
    assert same_bits(f.line_value(0.25), fresh.func_grad(x1 + 0.25 * d2, 0))


def test_planted_margins_behave_as_in_pass_one(acc):
    """the carried margins land on s = 0, -0.0, +-746, +-inf and NaN exactly: t and r are those of pass 1"""
    A, x, y, s = LN.planted(7, 129, 3, LN.PLANTED_SHORT)
    d = np.random.RandomState(9).randint(-3, 4, size=129).astype(np.float64)
    d[0] = 1.0
    x0 = x - 0.5 * d                                            # x0[0] = 0.5: the planted rows reach k at a = 0.5
    assert x0[0] == 0.5 and np.array_equal(x0 + 0.5 * d, x)
    f = exact_line(acc, A, x0, y, d, (0.5,))
    with np.errstate(invalid="ignore"):
        assert same_bits((y * f.fitted())[:s.size], s)
    t, r = f.losses(), f.weights()
    assert t[2] == 0.0 and r[2] == 0.0 and t[3] == 746.0 and r[3] == 1.0          # s = +-746 (y = +-1)
    assert t[4] == 0.0 and np.isnan(r[4]) and t[5] == np.inf and r[5] == np.inf     # s = +-inf
    assert np.isnan(t[6]) and np.isnan(r[6]) and np.isnan(f.func_grad_carried(0))


def step_bound(A, x, a, d):
    n = A.shape[1]
    Al = np.abs(A)
    return LN.gamma(LN.device_chain(n) + 2) * (Al.dot(np.abs(x)) + abs(a) * Al.dot(np.abs(d)))


def ld_value(A, y, xl):
    """(f, sum of the T_ULP allowances / m) at the np.longdouble point xl"""
    s = np.asarray(y, dtype=LD) * np.asarray(A, dtype=LD).dot(xl)
    t, _ = LN.tq_ref(s)
    return np.sum(t) / A.shape[0], float(np.sum(LN.ulps(LN.T_ULP, t))) / A.shape[0]


@pytest.mark.parametrize("m,n", [(96, 40), (33, 4100), (2050, 131)])
def test_general_data_value_within_the_derived_bound(acc, m, n):
    rng = np.random.RandomState(m + n)
    A, x, d = rng.randn(m, n), rng.randn(n) / np.sqrt(n), rng.randn(n) / np.sqrt(n)
    y = rng.choice([-1.0, 1.0], size=m)
    f = acc.LogisticRegression(A, y)
    f.func_grad(x, 2)
    f.line_begin(d)
    for a in (1.0, 0.37, -0.8, 1e-3):
        ref, allow = ld_value(A, y, np.asarray(x, dtype=LD) + LD(a) * np.asarray(d, dtype=LD))
        bound = float(np.sum(step_bound(A, x, a, d))) / m + allow
        err = abs(LD(f.line_value(a)) - ref)
        print("(%d,%d) a=%g: |df| %.3e, bound %.3e" % (m, n, a, float(err), bound))
        assert err <= bound


def test_general_data_after_63_carried_accepts(acc):
    m, n, k = 96, 40, 63
    rng = np.random.RandomState(7)
    A, x = rng.randn(m, n), rng.randn(n) / np.sqrt(n)
    y = rng.choice([-1.0, 1.0], size=m)
    f = acc.LogisticRegression(A, y)
    f.func_grad(x, 2)
    xl, total = np.asarray(x, dtype=LD), np.zeros(m)
    for j in range(k):
        d, a = rng.randn(n) / np.sqrt(n), rng.uniform(0.05, 0.5)
        total += step_bound(A, np.asarray(xl, dtype=np.float64), a, d)
        f.line_begin(d)
        f.line_accept(a)
        xl = xl + LD(a) * np.asarray(d, dtype=LD)
    ref, allow = ld_value(A, y, xl)
    bound = float(np.sum(total)) / m + allow
    err = abs(LD(f.func_grad_carried(0)) - ref)
    zerr = np.abs(LD(f.fitted()) - np.asarray(A, dtype=LD).dot(xl))
    print("after %d accepts: |df| %.3e, bound %.3e; margins at most %.3f of their bound" % (
        k, float(err), bound, float(np.max(zerr / total))))
    assert err <= bound and np.all(zerr <= total)


def test_stale_handles_are_refused(acc):
    A, x, y = LN.exact_data(33, 130, 4)
    d = np.ones(130)
    f = acc.LogisticRegression(A, y)
    for call in (lambda: f.line_begin(d), lambda: f.line_value(0.5), lambda: f.line_accept(0.5),
                 lambda: f.func_grad_carried(2)):
        with pytest.raises(ValueError):                         # no func_grad yet
            call()
    f.func_grad(x, 0)
    for call in (lambda: f.line_value(0.5), lambda: f.line_accept(0.5)):
        with pytest.raises(ValueError):                         # no line_begin yet
            call()
    f.line_begin(d)
    f.line_value(0.5)
    f.func_grad(x, 1)                                           # rebases the margins: the line is gone
    with pytest.raises(ValueError):
        f.line_value(0.5)
    f.line_begin(d)
    f.line_accept(0.5)
    with pytest.raises(ValueError):                             # an accepted step ends its line
        f.line_value(0.5)
    f.func_grad_carried(2)
    f.line_begin(d)
    with pytest.raises(AssertionError):
        f.line_begin(np.ones(5))
    with pytest.raises(AssertionError):
        f.func_grad_carried(3)
