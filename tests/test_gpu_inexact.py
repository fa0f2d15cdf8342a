"""GPU tests of the inexact-oracle accelerated methods AIBM, AdaptFGM and UniversalGM, of Poisson regression on the
simplex and of lmo_l2_ball_positive_orthant (accbpg/algorithms.py:593-777; accbpg/applications.py:209-295;
accbpg/functions_lmo.py:54-102) against tests/golden/inexact.npz, written by the real reference, and against the
NumPy restatement tests/inexact_numpy.py (which the CPU tests hold bit-equal to that fixture).

Per call.  Elementwise outputs (the combined point w, the LMO output, the accumulated gradient) are compared to rtol
1e-15; the two reductions of the combine kernel against the worst-case bound of a sequential sum, 2*n*eps*sum|terms|;
the fused prox must equal BurgEntropySimplex.prox_map on the same input bit for bit.

Trajectories.  These runs are not all digit-stable, so no tolerance is fixed in advance: the generator reran the
reference three times with its value and gradient perturbed at relative 1e-15 and stored, per run, the shortest
prefix on which F agreed to 1e-9 and G and the printed L to 1e-12, and the largest |x - x_rerun|.  Each run is pinned
here (F, G and the printed L, i.e. the line-search decisions) on half that prefix, which must be at least 30
iterations, and x to ten times the measured spread where the whole run agreed.  Measured (len / prefix / whole / x
spread), (2000,1000) seed 7 for the ten inexact-oracle runs, (300,500) seed 7 for the others:

    run              noise 0                         noise 1e-6
    AIBM gamma 2.0   80 / 63 / no                    80 / 63 / no
    AIBM gamma 1.4   80 / 80 / yes / 7.5e-10         80 / 80 / yes / 1.2e-11
    AIBM gamma 1.1   80 / 80 / yes / 2.3e-13         80 / 80 / yes / 1.5e-11
    AdaptFGM         80 / 70 / no                    80 / 70 / no
    UniversalGM      80 / 71 / no                    80 / 75 / no
    driver (placement x0_edge_sol_center): FW 120/120/yes/8.3e-16, BPG 120/120/yes/3.4e-21, BPG-LS 120/120/yes/4.4e-14,
    ABPG 120/120/yes/2.2e-16, ABPG_expo 120/72/no, ABPG_gain 120/120/yes/8.7e-11
    new LMO on Poisson_regrL2: FW_alg_div_step 120/120/yes/9.6e-15, FW_alg_descent_step 120/120/yes/5.9e-14

On the MI355X the pinned parts differ from the reference by at most 7.9e-12 in F (UniversalGM with noise; 1.6e-13 or
less elsewhere), by nothing in G and the printed L, and by a tenth to a half of the measured spread in x.  BPG without
line search started from an edge moved no bit of its near-1 entry in any rerun, so its measured spread (3.4e-21) is
the spacing of its 1e-5 entries; the bound on x is therefore never taken below the spacing of the format at the
largest entry compared.  b = np.dot(A, solution) depends on the host BLAS in its last bit: the rebuilt b is checked
to 1e-14 and the runs use the fixture's b, i.e. the reference's instance.
"""
import contextlib
import ctypes as C
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inexact_numpy as R  # noqa: E402

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SEED = 7
ACC = dict(m=2000, n=1000, noise=0.001)
ACC_ITERS = 80
FW = dict(m=300, n=500, noise=0.001)
FW_ITERS = 120
FW_PLACE = 'x0_edge_sol_center'
L2 = dict(m=300, n=500, noise=0.001, lamda=0.01, randseed=SEED, normalizeA=True)
L2_ITERS = 120
RUN_SEED = 1991
NOISES = [0, 1e-6]
GAMMAS = [2.0, 1.4, 1.1]
SIZES = [1, 2, 63, 64, 65, 1000, 4097, 65537, 300000]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def gold():
    return golden("inexact")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def odd(a):
    """a device copy whose base pointer is 8 bytes past the allocation's alignment"""
    buf = torch.empty(a.size + 1, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(np.ascontiguousarray(a))
    out = buf[1:]
    assert out.data_ptr() % 16 == 8
    return out


def _sum_tol(terms):
    """worst-case rounding of a sequential sum (the reference's) plus that of a tree sum (the device's)"""
    return 2 * len(terms) * EPS * float(np.sum(np.abs(terms))) + 1e-300


def _checksum(A):
    return np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()])


# ----------------------------------------------------------------------------------------------------- per call
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("place", [dev, odd])
def test_combine_ls_terms(acc, n, place):
    from accbpg_and_fw_amd.functions import combine_ls_terms
    rng = np.random.RandomState(n)
    u, v, x = rng.rand(n) + 0.05, rng.rand(n) + 0.05, rng.rand(n) + 0.05
    g = rng.randn(n)
    for h, c, a, b in [(acc.BurgEntropySimplex(), 1, 0.3, 0.7), (acc.BurgEntropy(), 1.7, 0.9, 2.1),
                       (acc.SquaredL2Norm(), 1, 0.3, 0.7), (acc.SquaredL2Norm(), 0.37, 1.3, 0.2)]:
        w, lin, dist = combine_ls_terms(h, a, place(u), b, place(v), c, place(g), place(x))
        assert isinstance(w, torch.Tensor) and w.is_cuda
        wr = (a * u + b * v) / c
        np.testing.assert_allclose(w.cpu().numpy(), wr, rtol=1e-15, atol=0)
        wn = w.cpu().numpy()
        lin_terms = g * (wn - x)
        print("n", n, "lin", lin, abs(lin - np.dot(g, wn - x)), _sum_tol(lin_terms))
        assert abs(lin - np.dot(g, wn - x)) <= _sum_tol(lin_terms)
        if isinstance(h, acc.SquaredL2Norm):
            terms = 0.5 * (wn - x) ** 2
            ref = 0.5 * np.vdot(wn - x, wn - x)
        else:
            r = wn / x
            terms = r - np.log(r) - 1
            ref = sum(terms)
        print("n", n, "dist", dist, abs(dist - ref), _sum_tol(terms))
        assert abs(dist - ref) <= _sum_tol(terms)
        # w alone: nothing reduced, same bits
        w2, none1, none2 = combine_ls_terms(h, a, place(u), b, place(v), c)
        assert none1 is None and none2 is None and torch.equal(w2, w)


def test_combine_asserts_positivity(acc):
    from accbpg_and_fw_amd.functions import combine_ls_terms
    u = dev(np.array([0.5, 0.2, 0.3]))
    x = dev(np.array([0.5, 0.0, 0.5]))
    with pytest.raises(AssertionError):
        combine_ls_terms(acc.BurgEntropySimplex(), 0.5, u, 0.5, u, 1, u, x)
    combine_ls_terms(acc.SquaredL2Norm(), 0.5, u, 0.5, u, 1, u, x)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("place", [dev, odd])
def test_fused_prox_equals_prox_map(acc, n, place):
    h = acc.BurgEntropySimplex(eps=1e-7)
    rng = np.random.RandomState(100 + n)
    xi, g = rng.randn(n) * 3, rng.randn(n)
    alpha = 0.37
    xi_out, z = h.prox_map_acc(place(xi), alpha, place(g))
    np.testing.assert_allclose(xi_out.cpu().numpy(), xi + alpha * g, rtol=1e-15, atol=0)
    same = h.prox_map(xi_out, 1)
    assert torch.equal(z, same)
    zr = R.BurgSimplexOracle(eps=1e-7).prox_map(xi_out.cpu().numpy(), 1)
    assert abs(float(z.sum()) - 1) < 1e-6
    np.testing.assert_allclose(z.cpu().numpy(), zr, rtol=1e-9, atol=0)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("place", [dev, odd])
def test_lmo_per_call(acc, n, place):
    rng = np.random.RandomState(200 + n)
    g = rng.randn(n)
    g[0] = -abs(g[0])
    c = rng.rand(n)
    for radius, center, eps, gg in [(1, None, 0.0, g), (0.7, c, 1e-7, g), (2.0, c + 0.5, 0.0, g),
                                    (1.5, c - 0.5, 1e-3, np.abs(g))]:
        ref = R.lmo_l2_ball_positive_orthant(radius, center, eps)(gg)
        got = acc.lmo_l2_ball_positive_orthant(radius, center, eps)(place(gg))
        assert isinstance(got, torch.Tensor) and got.is_cuda
        np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=1e-15, atol=0)
        got_np = acc.lmo_l2_ball_positive_orthant(radius, center, eps)(gg)
        assert isinstance(got_np, np.ndarray)
        np.testing.assert_array_equal(got_np, got.cpu().numpy())


def test_lmo_against_reference_outputs(acc, gold):
    for n in (1, 2, 63, 64, 65, 1000):
        g, c = gold["lmo_g_%d" % n], gold["lmo_c_%d" % n]
        for key, lmo, gg in [("s0", acc.lmo_l2_ball_positive_orthant(1), g),
                             ("s1", acc.lmo_l2_ball_positive_orthant(0.7, center=c, epsilon=1e-7), g),
                             ("s2", acc.lmo_l2_ball_positive_orthant(2.0, center=c + 0.5, epsilon=0.0), g),
                             ("pos", acc.lmo_l2_ball_positive_orthant(1.5, center=c - 0.5, epsilon=1e-3), np.abs(g))]:
            np.testing.assert_allclose(lmo(gg), gold["lmo_%s_%d" % (key, n)], rtol=1e-15, atol=0)


def test_lmo_assertions(acc):
    g = np.array([-1.0, 2.0, -3.0, 0.5])
    with pytest.raises(AssertionError, match="Shape mismatch between g and center"):
        acc.lmo_l2_ball_positive_orthant(1.0, center=np.zeros(3))(g)
    with pytest.raises(AssertionError, match="Output outside L2 ball"):
        acc.lmo_l2_ball_positive_orthant(1.0, epsilon=0.9)(g)          # lifting to 0.9 leaves the ball
    with pytest.raises(AssertionError, match="Output violates epsilon-nonnegativity"):
        acc.lmo_l2_ball_positive_orthant(1.0, center=np.array([np.nan, 0, 0, 0]))(g)
    # no negative entry: max(c, eps) and no assertion, even far outside the ball
    out = acc.lmo_l2_ball_positive_orthant(1.0, epsilon=50.0)(np.abs(g))
    np.testing.assert_array_equal(out, np.full(4, 50.0))


# ----------------------------------------------------------------------------------------------------- trajectories
def _printed(text, col=2):
    rows = [ln.split() for ln in text.splitlines() if ln[:6].strip().isdigit()]
    return np.array([int(r[0]) for r in rows]), np.array([float(r[col]) for r in rows])


def _run(call):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = call()
    return res, buf.getvalue()


def _pin(gold, key, x, F, G, text):
    """F, G and the printed L on half the prefix the reference reproduces under a 1e-15 perturbation of its oracle;
    x to ten times the reference's own spread where its whole run reproduces."""
    Fr, Gr, Lr, k0 = gold[key + "_F"], gold[key + "_G"], gold[key + "_Lk"], int(gold[key + "_k0"])
    prefix, whole, xspread = int(gold[key + "_prefix"]), bool(gold[key + "_whole"]), float(gold[key + "_xspread"])
    half = prefix // 2
    assert half >= 30, (key, prefix)
    ks, Lk = _printed(text)
    dF = np.abs(F[:half] - Fr[:half]) / (1 + np.abs(Fr[:half]))
    dG = np.abs(G[:half] - Gr[:half]) / (1 + np.abs(Gr[:half]))
    print("%-16s len %d/%d prefix %d pinned %d  dF %.2e dG %.2e" % (key, len(F), len(Fr), prefix, half, dF.max(),
                                                                   dG.max()), end="")
    assert len(F) >= half
    assert dF.max() <= 1e-9, (key, int(np.argmax(dF)))
    assert dG.max() <= 1e-12, (key, int(np.argmax(dG)))
    assert int(ks[0]) == k0
    np.testing.assert_allclose(Lk[:half - k0], Lr[:half - k0], rtol=1e-12, atol=0)
    lines = text.splitlines()
    assert list(gold[key + "_head"]) == lines[1:3], key
    ref_row, row = str(gold[key + "_row"]), lines[3]
    assert len(row) == len(ref_row) and row[:row.rindex(" ")] == ref_row[:ref_row.rindex(" ")], (row, ref_row)
    if whole:
        dx = float(np.max(np.abs(x - gold[key + "_x"])))
        print("  dx %.2e (spread %.2e)" % (dx, xspread))
        assert len(F) == len(Fr)
        # a spread cannot be resolved below the spacing of the format at the entries compared (BPG without line search
        # from an edge moved no bit of its near-1 entry in any rerun: measured 3.4e-21, the spacing of its 1e-5 entries)
        assert dx <= 10 * max(xspread, EPS * float(np.max(np.abs(gold[key + "_x"])))), key
    else:
        print("")


def _acc_calls(acc, f, h, L, x0):
    calls = {}
    for ni, noise in enumerate(NOISES):
        for gamma in GAMMAS:
            calls["aibm_g%02d_n%d" % (round(gamma * 10), ni)] = \
                lambda gamma=gamma, noise=noise: acc.AIBM(f, h, L, x0, gamma=gamma, maxitrs=ACC_ITERS, noise=noise)
        calls["fgm_n%d" % ni] = lambda noise=noise: acc.AdaptFGM(f, h, L, x0, maxitrs=ACC_ITERS, noise=noise)
        calls["ugm_n%d" % ni] = lambda noise=noise: acc.UniversalGM(f, h, L, x0, maxitrs=ACC_ITERS, noise_level=noise)
    return calls


def test_inexact_trajectories(acc, gold):
    np.random.seed(SEED)
    f, hs, L, x0 = acc.Poisson_regr_simplex_acc(**ACC)
    np.testing.assert_array_equal(_checksum(f.A), gold["acc_A_checksum"])
    np.testing.assert_array_equal(x0, gold["acc_x0"])
    # b = np.dot(A, solution) depends on the host BLAS to the last bit (the CPU tests pin it where the fixture was
    # written); the runs below are the reference's instance: its b and L
    np.testing.assert_allclose(f.b, gold["acc_b"], rtol=1e-14, atol=0)
    f, L = acc.PoissonRegression(f.A, gold["acc_b"]), float(gold["acc_L"])
    assert isinstance(hs[0], acc.BurgEntropySimplex) and hs[0].eps == 1e-7 and isinstance(hs[1], acc.SquaredL2Norm)
    for idx, (name, call) in enumerate(_acc_calls(acc, f, hs[0], L, x0).items()):
        np.random.seed(RUN_SEED + idx)
        (x, F, G, T), text = _run(call)
        assert np.random.random_sample() == float(gold["acc_%s_after" % name]), name      # same draws consumed
        assert isinstance(x, np.ndarray) and len(T) == len(F) == len(G)
        _pin(gold, "acc_" + name, x, F, G, text)


def test_inexact_device_x0_and_composed_loops(acc, gold):
    """a device x0 gives device results with the same numbers, and the loops composed from the public kernels
    (FUSED_INEXACT = False) take the same decisions"""
    from accbpg_and_fw_amd import algorithms
    np.random.seed(SEED)
    f, hs, L, x0 = acc.Poisson_regr_simplex_acc(**ACC)
    f, L = acc.PoissonRegression(f.A, gold["acc_b"]), float(gold["acc_L"])
    for name, call in [("aibm", lambda x: acc.AIBM(f, hs[0], L, x, gamma=1.4, maxitrs=30, verbose=False)),
                       ("fgm", lambda x: acc.AdaptFGM(f, hs[0], L, x, maxitrs=30, verbose=False)),
                       ("ugm", lambda x: acc.UniversalGM(f, hs[0], L, x, maxitrs=30, verbose=False))]:
        xn, Fn, Gn, _ = call(x0)
        xd, Fd, Gd, _ = call(dev(x0))
        assert isinstance(xd, torch.Tensor) and xd.is_cuda
        np.testing.assert_array_equal(xd.cpu().numpy(), xn)
        np.testing.assert_array_equal(Fd, Fn)
        algorithms.FUSED_INEXACT = False
        try:
            xc, Fc, Gc, _ = call(x0)
        finally:
            algorithms.FUSED_INEXACT = True
        np.testing.assert_allclose(Fc, Fn, rtol=1e-9)
        np.testing.assert_allclose(Gc, Gn, rtol=1e-12)
        np.testing.assert_allclose(xc, xn, rtol=0, atol=1e-10)


def test_fw_driver_six_calls(acc, gold):
    np.random.seed(SEED)
    h, places = acc.Poisson_regr_simplex(**FW)
    assert list(places) == list(R.PLACEMENTS) and isinstance(h, acc.BurgEntropySimplex) and h.eps == 1e-8
    for key, (fk, Lk, sol, x0k) in places.items():
        np.testing.assert_array_equal(_checksum(fk.A), gold["fw_%s_A_checksum" % key])
        np.testing.assert_allclose(fk.b, gold["fw_%s_b" % key], rtol=1e-14, atol=0)      # host BLAS, see above
        np.testing.assert_array_equal(x0k, gold["fw_%s_x0" % key])
        np.testing.assert_array_equal(sol, gold["fw_%s_sol" % key])
        np.testing.assert_allclose(Lk, float(gold["fw_%s_L" % key]), rtol=1e-14)
    f, L, sol, x0 = places[FW_PLACE]
    f, L = acc.PoissonRegression(f.A, gold["fw_%s_b" % FW_PLACE]), float(gold["fw_%s_L" % FW_PLACE])
    N = FW_ITERS
    calls = {
        "fw": lambda: acc.FW_alg_div_step(f, h, L, x0, lmo=acc.lmo_simplex(1), maxitrs=N, gamma=2.0, ls_ratio=1.5)[:3],
        "bpg": lambda: acc.BPG(f, h, L, x0, maxitrs=N, linesearch=False)[:3],
        "bpgls": lambda: acc.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5)[:3],
        "abpg": lambda: acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=False)[:3],
        "expo": lambda: (lambda r: (r[0], r[1], r[3]))(acc.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=N, theta_eq=False,
                                                                     Gmargin=1)),
        "gain": lambda: acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, ls_inc=1.5, ls_dec=1.5,
                                      theta_eq=True)[:3],
    }
    for idx, (name, call) in enumerate(calls.items()):
        np.random.seed(RUN_SEED + idx)
        (x, F, G), text = _run(call)
        _pin(gold, "fw_" + name, x, F, G, text)


def test_new_lmo_inside_frank_wolfe(acc, gold):
    f, h, L, x0 = acc.Poisson_regrL2(**L2)
    np.testing.assert_allclose(f.b, gold["l2_b"], rtol=1e-14, atol=0)
    f = acc.PoissonRegression(f.A, gold["l2_b"])
    L = gold["l2_b"].sum()
    lmo = acc.lmo_l2_ball_positive_orthant(1, epsilon=1e-7)
    calls = {
        "l2div": lambda: acc.FW_alg_div_step(f, h, L, x0, maxitrs=L2_ITERS, gamma=2.0, lmo=lmo)[:3],
        "l2desc": lambda: (lambda r: (r[0], r[1], r[3]))(acc.FW_alg_descent_step(f, h, x0, maxitrs=L2_ITERS, lmo=lmo)),
    }
    for idx, (name, call) in enumerate(calls.items()):
        np.random.seed(RUN_SEED + idx)
        (x, F, G), text = _run(call)
        _pin(gold, "l2_" + name, x, F, G, text)


# ----------------------------------------------------------------------------------------------------- behaviour
class _NeverPasses:
    """an f whose line-search test cannot pass: its value alone (flag 0, the left side of every test) is +inf after
    the first `passes` such calls, the value that comes with a gradient (the right side) is 1"""

    def __init__(self, n, passes=0):
        self.n, self.passes = n, passes

    def func_grad(self, x, flag=2):
        g = torch.ones(self.n, dtype=torch.float64, device="cuda")
        if flag == 0:
            self.passes -= 1
            return 0.0 if self.passes >= 0 else float("inf")
        return g if flag == 1 else (1.0, g)

    def __call__(self, x):
        return self.func_grad(x, 0)

    def gradient(self, x):
        return self.func_grad(x, 1)


def test_non_finite_L_raises(acc):
    """Run on the Euclidean kernel: as L grows the step underflows and the iterates leave the positive orthant, where
    the Burg divergence asserts (as the reference's does) long before L is infinite.  L is a NumPy scalar, as the
    factories return it, so that AIBM's alpha/B overflows instead of raising ZeroDivisionError.  AIBM is stopped in
    its first search (passes=0) and in its main loop (passes=1)."""
    x0 = np.ones(8) / 8
    h = acc.SquaredL2Norm()
    L = np.float64(1.0)
    for call, passes in ((lambda f: acc.AIBM(f, h, L, x0, gamma=2.0, maxitrs=5, verbose=False), 0),
                         (lambda f: acc.AIBM(f, h, L, x0, gamma=2.0, maxitrs=5, verbose=False), 1),
                         (lambda f: acc.AIBM(f, acc.BurgEntropySimplex(eps=1e-7), L, x0, gamma=2.0, maxitrs=5,
                                             verbose=False), 0),
                         (lambda f: acc.AdaptFGM(f, h, L, x0, maxitrs=5, verbose=False), 0),
                         (lambda f: acc.UniversalGM(f, h, L, x0, maxitrs=5, verbose=False), 0)):
        with np.errstate(all="ignore"), pytest.raises(ValueError, match="L cannot be None or infinity"):
            call(_NeverPasses(8, passes))


def test_steps_generators_match_the_drained_calls(acc):
    np.random.seed(SEED)
    f, hs, L, x0 = acc.Poisson_regr_simplex_acc(60, 40, noise=0.001)
    from accbpg_and_fw_amd import algorithms
    for steps, full, kw in [(algorithms.AIBM_steps, acc.AIBM, dict(gamma=1.4)), (algorithms.AdaptFGM_steps, acc.AdaptFGM, {}),
                            (algorithms.UniversalGM_steps, acc.UniversalGM, {})]:
        gen = steps(f, hs[0], L, x0, maxitrs=6, verbose=False, **kw)
        seen = []
        while True:
            try:
                seen.append(next(gen))
            except StopIteration as stop:
                res = stop.value
                break
        ref = full(f, hs[0], L, x0, maxitrs=6, verbose=False, **kw)
        assert len(ref[1]) == 6 and seen == [1, 2, 3, 4, 5]          # no early stop in six iterations here
        np.testing.assert_array_equal(res[1], ref[1])
        np.testing.assert_array_equal(res[0], ref[0])
