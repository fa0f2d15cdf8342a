"""GPU tests of symmetric NMF (FrobeniusSymLoss, SumOf2nd4thPowers(PositiveOrthant), SquaredL2Norm, lmo_l2_ball,
lmo_linf_ball, FW_alg_descent_step; parameters_free_fw/ipynb/ex_SymNMF.ipynb): per-call parity with the fixture
written by the real reference, the M X product over an (n, r) grid that reaches every tail and launch plan, the
C-ABI with ldm > n, the reference's assertions, device residency, bit-identical repeats, the notebook's solver calls
with their printed rows, and f and g at (16384, 64) against host NumPy.

Tolerances.  f is a difference of terms of size ||M||_F^2 (about 1e16 at the notebook sizes), so values are compared
relative to ||M||_F^2.  Gradients and prox maps are compared relative to their largest entry; the prox maps at
L = 1 go through a cancelling cubic, where the reference moves by 1e-12 under a change of summation order alone.  Replaying the
notebook's trajectories with M X summed in another order (tests/symnmf_numpy.py, order=1) reproduces the
reference's F and L_k sequences exactly over all 200 iterations, so F is pinned to 1e-12 ||M||_F^2 and every
accept/reject decision (the L_k sequence) while F still moves by more than 1e-13 ||M||_F^2 per step; after that the
line search compares equal values and its decisions are left free."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symnmf_numpy as S  # noqa: E402

pytestmark = pytest.mark.gpu

RADIUS = 500.0
INSTANCES = [("l2_400", "l2", 400, 50, 1), ("linf_400", "linf", 400, 50, 2), ("linf_700", "linf", 700, 50, 3)]
PROX_L = [1.0, 1e3, 1e6]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def cs(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum()])


def inputs(n, r, seed):
    rng = np.random.RandomState(1000 + seed)
    return rng.rand(n, r) * 2 * RADIUS, rng.randn(n, r) * 1e9


def close_mat(gd, key, a, tol, scale=None):
    """a against the fixture's first rows and checksums, entrywise to tol * scale (default: the largest entry)."""
    a = np.asarray(a)
    rows = gd[key + "_rows"]
    if scale is None:
        scale = np.abs(rows).max() + 1e-300
    e = tol * scale
    assert np.max(np.abs(a[:rows.shape[0]] - rows)) <= e, key
    got, want = cs(a), gd[key + "_cs"]
    bound = [a.size * e, a.size * e, 2 * e * want[1] + a.size * e * e]
    assert np.all(np.abs(got - want) <= np.array(bound) + 1e-300), (key, got, want)


def build(acc, kind, n, r, seed):
    np.random.seed(seed)
    center = np.ones((n, r)) * RADIUS
    fac = acc.FrobeniusSymLossExL2Ball if kind == "l2" else acc.FrobeniusSymLossExLInfBall
    f, h, L, X0, M = fac(n, r, center, radius=RADIUS, on_boundary=False)
    lmo = (acc.lmo_l2_ball if kind == "l2" else acc.lmo_linf_ball)(RADIUS, center=center)
    return f, h, L, X0, M, lmo, center


# ------------------------------------------------------------------ per-call parity
@pytest.mark.parametrize("tag,kind,n,r,seed", INSTANCES)
def test_percall_parity(acc, tag, kind, n, r, seed):
    gd = golden("symnmf")
    f, h, L, X0, M, lmo, center = build(acc, kind, n, r, seed)
    np.testing.assert_allclose(cs(M), gd[tag + "_M_cs"], rtol=1e-13)
    assert h.sigma == pytest.approx(float(gd[tag + "_sigma"]), rel=1e-13)
    nm2 = f.M_norm ** 2
    X, G = inputs(n, r, seed)
    for pt, P in (("x0", X0), ("xr", X)):
        fx, g = f.func_grad(P, 2)
        assert isinstance(g, np.ndarray) and g.shape == (n, r)
        assert abs(fx - gd["%s_%s_f" % (tag, pt)]) <= 1e-13 * nm2
        assert abs(f(P) - fx) == 0
        # g = 2 X S - 2 M X cancels at X0: compared relative to the size of its two terms
        gscale = 2 * np.abs(P @ (P.T @ P)).max() + 2 * np.abs(M @ P).max()
        close_mat(gd, "%s_%s_g" % (tag, pt), g, 1e-13, gscale)
    hs = {"q": h, "qo": acc.SumOf2nd4thPowersPositiveOrthant(h.alpha, h.sigma),
          "qu": acc.SumOf2nd4thPowersPositiveOrthant(h.alpha, h.sigma, upper_bound=RADIUS)}
    for name, hh in hs.items():
        for i, Lp in enumerate(PROX_L):
            # (at L = 1 the cubic's b - sqrt(delta)/2 cancels: summing ||y||^2 in reverse order moves the
            # reference's own result by 1.05e-12 of its largest entry)
            close_mat(gd, "%s_prox_%s_%d" % (tag, name, i), hh.div_prox_map(X, G, Lp), 1e-11)
    assert h(X) == pytest.approx(float(gd[tag + "_h_x"]), rel=1e-13)
    close_mat(gd, tag + "_h_grad", h.gradient(X), 1e-13)
    hx = float(gd[tag + "_h_x"])
    for got, want in zip([h.divergence(X, X0), h.divergence(X0, X)], gd[tag + "_div"]):
        assert abs(got - want) <= 1e-13 * hx
    for c, want in zip((1e-3, 1.0, 1e12, 1e30), gd[tag + "_cubic"]):
        assert h.solve_cubic(c, h.sigma) == want
    close_mat(gd, tag + "_lmo_g", lmo(G), 1e-13)
    np.testing.assert_allclose(cs(lmo(np.zeros((n, r)))), gd[tag + "_lmo_zero"], rtol=1e-15)
    close_mat(gd, tag + "_lmo_l2_scalar", acc.lmo_l2_ball(RADIUS, center=1)(G), 1e-13)
    close_mat(gd, tag + "_lmo_l2_none", acc.lmo_l2_ball(RADIUS)(G), 1e-13)
    Gz = G.copy()
    Gz[:, 0] = 0.0
    close_mat(gd, tag + "_lmo_linf_scalar", acc.lmo_linf_ball(1, center=1)(Gz), 0)
    close_mat(gd, tag + "_lmo_linf_none", acc.lmo_linf_ball(RADIUS)(Gz), 0)


def test_resmeas_parity(acc):
    gd = golden("symnmf")
    np.random.seed(4)
    B = np.random.rand(300, 30)
    M = B @ B.T
    f, (h, h_euk), L, X0 = acc.FrobeniusSymLossResMeasEx(M, 70)
    np.testing.assert_allclose(cs(M), gd["rm_M_cs"], rtol=1e-13)
    np.testing.assert_allclose(cs(X0), gd["rm_X0_cs"], rtol=1e-15)
    assert isinstance(h, acc.SumOf2nd4thPowersPositiveOrthant) and h.upper_bound is None
    nm2 = f.M_norm ** 2
    assert abs(f(X0) - gd["rm_f0"]) <= 1e-13 * nm2
    X, G = inputs(300, 70, 4)
    np.testing.assert_allclose([h_euk(X), h_euk.divergence(X, X0)], gd["rm_euk"], rtol=1e-13)
    close_mat(gd, "rm_euk_prox", h_euk.div_prox_map(X, G, 1e6), 1e-15)
    # every BPG / ABPG step goes through the prox map's cancelling cubic: F is compared to 1e-10 ||M||_F^2
    x, F, Ls, _ = acc.BPG(f, h, L, X0, maxitrs=50, linesearch=False, verbose=False)
    assert x.shape == X0.shape and isinstance(x, np.ndarray)
    assert len(F) == len(gd["rm_bpg_F"]) and np.max(np.abs(F - gd["rm_bpg_F"])) <= 1e-10 * nm2
    np.testing.assert_allclose(cs(x), gd["rm_bpg_x"], rtol=1e-8)
    x, F, G_, _ = acc.ABPG(f, h, L, X0, gamma=2.0, maxitrs=50, theta_eq=True, restart=False, verbose=False)
    assert len(F) == len(gd["rm_abpg_F"]) and np.max(np.abs(F - gd["rm_abpg_F"])) <= 1e-10 * nm2
    np.testing.assert_allclose(cs(x), gd["rm_abpg_x"], rtol=1e-8)


# ------------------------------------------------------------------ the M X product
_MCACHE = {}


def _sym(n):
    if n not in _MCACHE:
        _MCACHE.clear()
        g = torch.Generator(device="cuda").manual_seed(n)
        A = torch.rand(n, n, dtype=torch.float64, device="cuda", generator=g)
        _MCACHE[n] = (A + A.T) * 0.5
        del A
    return _MCACHE[n]


def _expect(M, X):
    """f and g in torch fp64 (an independent summation order)."""
    MX = M @ X
    Sx = X.T @ X
    f = 0.5 * (float(torch.linalg.norm(M)) ** 2 + float(torch.linalg.norm(Sx)) ** 2) - float((X * MX).sum())
    return f, 2 * (X @ Sx) - 2 * MX


@pytest.mark.parametrize("n", [1, 17, 400, 4097, 16384])
def test_product_grid(acc, n):
    M = _sym(n)
    for r in (1, 3, 16, 50, 64, 70, 128, 130):
        X = torch.rand(n, r, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(r))
        f = acc.FrobeniusSymLoss(M, X)
        fx, g = f.func_grad(X)
        assert g.is_cuda and g.shape == (n, r)
        fe, ge = _expect(M, X)
        scale = 0.5 * f.M_norm ** 2 + float((X * X).sum()) ** 2
        assert abs(fx - fe) <= 1e-13 * scale + 1e-300, (n, r, fx, fe)
        gscale = float(ge.abs().max()) + float((2 * (X @ (X.T @ X))).abs().max())
        assert float((g - ge).abs().max()) <= 1e-13 * gscale, (n, r)
        assert f(X) == fx
        assert torch.equal(f.gradient(X), g)
        nsplit, kchunk, wide, gchunks = f.plan()
        assert wide == (1 if r > 64 else 0) and nsplit * kchunk >= n > (nsplit - 1) * kchunk and kchunk % 16 == 0


def test_plans_reach_split_and_single(acc):
    plans = {}
    for n, r in ((400, 50), (4097, 70), (16384, 64), (16384, 130)):
        M = _sym(n)
        plans[(n, r)] = acc.FrobeniusSymLoss(M, torch.zeros(n, r, dtype=torch.float64, device="cuda")).plan()
    assert plans[(400, 50)][0] == 1
    assert plans[(4097, 70)][0] > 1 and plans[(16384, 64)][0] > 1
    assert plans[(16384, 130)][2] == 1


def test_capi_ldm_greater_than_n(acc):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    for n, r, pad in ((300, 50, 5), (1000, 70, 3), (517, 3, 1)):
        rng = np.random.RandomState(n)
        A = rng.rand(n, n)
        M = (A + A.T) / 2
        big = np.full((n, n + pad), np.nan)
        big[:, :n] = M
        Md = dev(big)
        X = rng.rand(n, r)
        Xd = dev(X)
        h = C.c_void_p()
        mn = np.linalg.norm(M)
        assert lib.accbpg_symnmf_create(C.c_void_p(Md.data_ptr()), n, n + pad, r, mn, None, C.byref(h)) == 0
        g = torch.empty(n, r, dtype=torch.float64, device="cuda")
        fv = C.c_double()
        assert lib.accbpg_symnmf_func_grad(h, C.c_void_p(Xd.data_ptr()), 2, C.byref(fv), C.c_void_p(g.data_ptr())) == 0
        lib.accbpg_symnmf_destroy(h)
        fr, gr = S.FrobeniusSymLoss(M, X).func_grad(X)
        fscale = mn ** 2 + np.sum(X * X) ** 2
        assert abs(fv.value - fr) <= 1e-13 * fscale
        assert np.max(np.abs(g.cpu().numpy() - gr)) <= 1e-12 * np.abs(gr).max()
        # a device M with a padded row stride is borrowed as it is
        f = acc.FrobeniusSymLoss(Md[:, :n], X)
        assert f._M.stride(0) == n + pad
        assert abs(f(X) - fr) <= 1e-13 * fscale
    bad = C.c_void_p()
    assert lib.accbpg_symnmf_create(C.c_void_p(Md.data_ptr()), n, n - 1, r, 1.0, None, C.byref(bad)) == _lib.ERR_ARG


# ------------------------------------------------------------------ assertions, residency, repeats
def test_assertions(acc):
    rng = np.random.RandomState(0)
    M = rng.rand(20, 20)
    with pytest.raises(AssertionError, match="Matrix M must be symmetric."):
        acc.FrobeniusSymLoss(M, np.ones((20, 3)))
    with pytest.raises(AssertionError, match="Matrix M must be symmetric."):
        acc.FrobeniusSymLoss(dev(M), np.ones((20, 3)))
    Ms = M + M.T
    f = acc.FrobeniusSymLoss(Ms, np.ones((20, 3)))
    with pytest.raises(AssertionError):
        f(np.ones((20, 4)))
    h = acc.SumOf2nd4thPowers(6, 1.0)
    with pytest.raises(AssertionError, match="Bregman div: x and y not same shape."):
        h.divergence(np.ones((20, 3)), np.ones((20, 4)))
    with pytest.raises(AssertionError, match="Vectors y and g not same shape."):
        acc.SquaredL2Norm().div_prox_map(np.ones(3), np.ones(4), 1.0)
    # far from the origin the rounding of c - s breaks the reference's boundary check too
    g = rng.randn(50, 4)
    with pytest.raises(AssertionError, match="Solution does not lie on ball boundary"):
        S.lmo_l2_ball(1.0, center=1e9)(g)
    with pytest.raises(AssertionError, match="Solution does not lie on ball boundary"):
        acc.lmo_l2_ball(1.0, center=1e9)(g)


def test_device_tensors_stay_on_device(acc):
    f, h, L, X0, M, lmo, center = build(acc, "linf", 400, 50, 2)
    Xd = dev(X0)
    fx, g = f.func_grad(Xd)
    assert isinstance(fx, np.floating) and g.is_cuda and g.shape == Xd.shape
    for out in (lmo(g), acc.lmo_l2_ball(RADIUS, dev(center))(g), h.div_prox_map(Xd, g, 1.0), h.gradient(Xd),
                acc.SquaredL2Norm().div_prox_map(Xd, g, 1.0), acc.lmo_linf_ball(1, center=1)(g)):
        assert isinstance(out, torch.Tensor) and out.is_cuda and out.shape == Xd.shape
    for call in (lambda: acc.FW_alg_div_step(f, h, L, Xd, 3, 2.0, lmo, verbose=False)[0],
                 lambda: acc.FW_alg_descent_step(f, h, Xd, 3, lmo, verbose=False)[0],
                 lambda: acc.BPG(f, h, L, Xd, 3, linesearch=False, verbose=False)[0],
                 lambda: acc.ABPG(f, h, L, Xd, 2.0, 3, verbose=False)[0]):
        x = call()
        assert isinstance(x, torch.Tensor) and x.is_cuda and x.shape == Xd.shape


def test_bit_identical_repeats(acc):
    for n, r in ((4097, 70), (16384, 64), (700, 50)):
        M = _sym(n)
        X = torch.rand(n, r, dtype=torch.float64, device="cuda")
        f = acc.FrobeniusSymLoss(M, X)
        a = f.func_grad(X)
        b = f.func_grad(X)
        assert a[0] == b[0] and torch.equal(a[1], b[1])
    h = acc.SumOf2nd4thPowersPositiveOrthant(6, 10.0)
    G = torch.randn(n, r, dtype=torch.float64, device="cuda")
    assert torch.equal(h.div_prox_map(X, G, 3.0), h.div_prox_map(X, G, 3.0))
    assert h.divergence(X, G) == h.divergence(X, G)
    lmo = acc.lmo_l2_ball(2.0)
    assert torch.equal(lmo(G), lmo(G))


def test_fw_descent_single_iteration(acc):
    f, h, L, X0, M, lmo, center = build(acc, "linf", 400, 50, 2)
    x, F, T, G = acc.FW_alg_descent_step(f, h, X0, 1, lmo, verbose=False)
    assert len(F) == len(T) == len(G) == 1 and F[0] == f(X0) and np.array_equal(x, X0)


def test_noise_draws_follow_the_legacy_rng(acc):
    f, h, L, X0, M, lmo, center = build(acc, "linf", 400, 50, 2)
    fn = acc.FrobeniusSymLoss(M, X0, noise_level=0.1)
    np.random.seed(7)
    g = fn.gradient(X0)
    np.random.seed(7)
    noise = (np.random.randn(*X0.shape) - 0.5) * 0.1
    np.testing.assert_allclose(g, f.gradient(X0) + noise, rtol=0, atol=1e-12 * np.abs(g).max())


# ------------------------------------------------------------------ the notebook's solver calls
def _rows(txt):
    """printed rows without the time column"""
    return [re.sub(r"\s+\S+\s*$", "", ln) if re.match(r"\s+\d+\s", ln) else ln for ln in txt]


@pytest.mark.parametrize("tag,kind,n,r,seed", INSTANCES)
def test_notebook_trajectories(acc, capsys, tag, kind, n, r, seed):
    gd = golden("symnmf")
    f, h, L, X0, M, lmo, center = build(acc, kind, n, r, seed)
    nm2 = np.linalg.norm(M) ** 2
    capsys.readouterr()
    for key, call in (("fwls", lambda: acc.FW_alg_div_step(f, h, L, X0, maxitrs=200, gamma=2.0, lmo=lmo,
                                                          linesearch=True, ls_ratio=2.0, verbskip=50)),
                      ("fw", lambda: acc.FW_alg_div_step(f, h, L, X0, maxitrs=200, gamma=2.0, lmo=lmo,
                                                        linesearch=False, verbskip=50)),
                      ("desc", lambda: acc.FW_alg_descent_step(f, h, X0, maxitrs=200, lmo=lmo, verbskip=50))):
        x, F, third, _ = call()
        txt = capsys.readouterr().out.splitlines()
        assert x.shape == X0.shape
        rF = gd[tag + "_%s_F" % key]
        # the reference stops on |F[k] - F[k-1]| < 1e-14 with F ~ 1e16: at an exactly stationary F, a last-bit
        # decision (l2_400 without line search stops at k = 28, this run a few steps later); F is pinned on the
        # common prefix and a different length is accepted only at such a point
        m = min(len(F), len(rF))
        assert np.max(np.abs(F[:m] - rF[:m])) <= 1e-12 * nm2, key
        if len(F) != len(rF):
            assert abs(rF[-1] - rF[-2]) < 1e-14 and np.all(np.abs(np.diff(F[m - 1:])) <= 1e-13 * nm2), key
        if key != "desc":
            # decisions are pinned while the steps still move F: once F is stationary (the l2 line search ends
            # that way: 14 of its 18 iterations are pinned) the test compares equal values and the last bit decides
            moving = np.nonzero(np.abs(np.diff(rF)) < 1e-13 * nm2)[0]
            k_pin = int(moving[0]) + 1 if moving.size else len(rF)
            k_pin = min(k_pin, m)
            np.testing.assert_array_equal(third[:k_pin], gd[tag + "_%s_Ls" % key][:k_pin])
            assert k_pin >= 14, k_pin
        # (after free decisions the final point moves by the tiny steps they take: 2.4e-8 at l2_400)
        xtol = 1e-10 if len(F) == len(rF) and (key == "desc" or k_pin == len(rF)) else 1e-7
        np.testing.assert_allclose(cs(x), gd[tag + "_%s_x" % key], rtol=xtol, err_msg=key)
        want = _rows(list(gd[tag + "_%s_rows" % key]))
        assert _rows(txt)[:len(want)] == want, key
        if kind == "l2":
            assert np.linalg.norm(x - center, 2) <= RADIUS + 1e-6
        else:
            assert np.max(np.abs(x - center)) <= RADIUS + 1e-6


# ------------------------------------------------------------------ properties at (16384, 64)
def test_large_against_host_numpy(acc):
    n, r = 16384, 64
    M = _sym(n)
    rng = np.random.RandomState(5)
    X = rng.rand(n, r)
    f = acc.FrobeniusSymLoss(M, X)
    fx, g = f.func_grad(X)
    Mh = M.cpu().numpy()
    fr, gr = S.FrobeniusSymLoss(Mh, X).func_grad(X)
    del Mh
    assert abs(fx - fr) <= 1e-13 * f.M_norm ** 2
    assert np.max(np.abs(g - gr)) <= 1e-12 * np.abs(gr).max()
    assert f(X) == fx
