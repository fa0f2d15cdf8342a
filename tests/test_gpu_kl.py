"""GPU tests of KL-divergence nonnegative regression with the Shannon-entropy kernels (accbpg/functions.py:123-158,
398-490; ipynb/ex_KL_regr_L1.ipynb): per-call parity with the fixture written by the real reference, func_grad at
the shapes that reach each branch of the A x kernel, the C-ABI with lda > n, the reference's assertions, the Shannon
kernels from n = 1 to 300000, the notebook's six solver calls, and properties at (8192, 65536).

Tolerances.  The matrix-vector products differ from BLAS by summation order (1e-13 relative).  The device exp and
log are not guaranteed to round like NumPy's: the prox maps are compared to rtol 1e-15 (a few ulp).  Sums over n
(simplex normalisation, divergences) are compared against the worst-case bound of a sequential sum, n * eps times the
sum of magnitudes.  Late in a run D(x+,y) is pure cancellation and the reference does not reproduce itself there
(a change of summation order alone moves ABPG's TSG after about 100-240 iterations, and BPG-LS amplifies rounding
until its L_k sequence splits at k = 20), so G is pinned on a prefix only; x and F are pinned throughout, at the
tolerances that the reference's own spread allows (test_kl_notebook_trajectories)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from conftest import golden

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kl_numpy as K  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [("s1", 1000, 100), ("s2", 100, 1000)]
ARGS = dict(noise=0.01, lamdaL1=0.001, randseed=1)
EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _close(a, b, tol):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


def _agree_prefix(a, b, tol):
    """length of the common prefix on which two traces agree to tol"""
    n = min(len(a), len(b))
    bad = np.nonzero(np.abs(a[:n] - b[:n]) > tol * (1 + np.abs(b[:n])))[0]
    return n if bad.size == 0 else int(bad[0])


def _sum_tol(terms):
    """worst-case rounding of a sequential sum (the reference's) plus that of a tree sum (the device's)"""
    return 2 * len(terms) * EPS * float(np.sum(np.abs(terms))) + 1e-300


def _kernels(acc):
    return [("sh", acc.ShannonEntropy(), K.Shannon()), ("l1", acc.ShannonEntropyL1(ARGS["lamdaL1"]),
                                                         K.ShannonL1(ARGS["lamdaL1"])),
            ("sx", acc.ShannonEntropySimplex(), K.ShannonSimplex())]


# ------------------------------------------------------------------ per call
@pytest.mark.parametrize("tag,m,n", SIZES)
def test_kl_percall_matches_reference_golden(acc, tag, m, n):
    gd = golden("kl")
    f, h, L, x0 = acc.KL_nonneg_regr(m, n, **ARGS)
    assert isinstance(f, acc.KLdivRegression) and isinstance(h, acc.ShannonEntropyL1) and h.lamda == 0.001
    assert L == gd[tag + "_L"]
    np.testing.assert_array_equal(f.b, gd[tag + "_b"])
    np.testing.assert_array_equal(x0, gd[tag + "_x0"])
    np.testing.assert_allclose([f.A.sum(), np.abs(f.A).max(), (f.A ** 2).sum()], gd[tag + "_A_checksum"], rtol=1e-13)
    x, y, gref = gd[tag + "_x"], gd[tag + "_y"], gd[tag + "_g"]
    fx, g = f.func_grad(x, 2)
    assert fx == pytest.approx(float(gd[tag + "_f"]), rel=1e-13)
    np.testing.assert_allclose(g, gref, rtol=1e-12, atol=1e-13 * np.abs(gref).max())
    assert f(x) == fx
    np.testing.assert_array_equal(f.gradient(x), g)
    assert f(x0) == pytest.approx(float(gd[tag + "_f0"]), rel=1e-13)
    g0 = gd[tag + "_g0"]
    np.testing.assert_allclose(f.gradient(x0), g0, rtol=1e-12, atol=1e-13 * np.abs(g0).max())
    np.testing.assert_allclose(f.fitted(), f.A @ x0, rtol=1e-13)
    assert h.extra_Psi(x) == pytest.approx(float(gd[tag + "_psi"]), rel=1e-14)
    for kname, hk, _ in _kernels(acc):
        # elementwise maps to a few ulp; the simplex maps also divide by a sum over n taken in another order
        tol = 1e-15 + (2 * n * EPS if kname == "sx" else 0.0)
        for idx, Lc in enumerate(gd[tag + "_prox_L"]):
            np.testing.assert_allclose(hk.prox_map(gref, Lc), gd["%s_%s_prox%d" % (tag, kname, idx)], rtol=tol)
            np.testing.assert_allclose(hk.div_prox_map(y, gref, Lc), gd["%s_%s_divprox%d" % (tag, kname, idx)],
                                       rtol=tol)
        dxy = hk.divergence(x, y)
        assert isinstance(dxy, np.float64)
        assert dxy == pytest.approx(float(gd["%s_%s_div_xy" % (tag, kname)]), rel=1e-13)
        dz = hk.divergence(gd[tag + "_xz"], gd[tag + "_yz"])
        assert dz == pytest.approx(float(gd["%s_%s_div_zero" % (tag, kname)]), rel=1e-13)


# ------------------------------------------------------------------ func_grad branches
def _against_restatement(acc, A, b, x, rtol_f=1e-13):
    fo, go = K.KLdiv(A, b).func_grad(x, 2)
    f = acc.KLdivRegression(A, b)
    fx, g = f.func_grad(x, 2)
    assert fx == pytest.approx(fo, rel=rtol_f)
    np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-12 * np.abs(go).max())
    assert f(x) == fx
    return f


@pytest.mark.parametrize("shape", [(37, 51), (1000, 3), (513, 1001), (64, 5001), (5, 4096), (300, 8192)])
def test_kl_shapes_against_restatement(acc, shape):
    """Odd sizes (scalar-load path), few long rows (workgroup-per-row path, m < 8 CUs' rows and n >= 4096)."""
    m, n = shape
    rng = np.random.RandomState(m + 7 * n)
    A = rng.rand(m, n)
    b = rng.rand(m) + 0.1
    x = rng.rand(n) / n + 1e-4
    _against_restatement(acc, A, b, x)


def test_kl_long_rows_branch_against_restatement(acc):
    """(2048, 32768): the wave-per-row A x kernel with its occupancy-limiting LDS request."""
    m, n = 2048, 32768
    rng = np.random.RandomState(13)
    A = rng.rand(m, n)
    b = rng.rand(m) * 0.5 + 0.25
    x = rng.rand(n) / n + 1e-5
    f = _against_restatement(acc, A, b, x, rtol_f=1e-12)
    np.testing.assert_allclose(f.fitted(), A @ x, rtol=1e-12)


def test_kl_leading_dimension_through_c_abi(acc):
    """lda > n and an unaligned base pointer, straight through the C-ABI."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n, lda = 70, 301, 333
    rng = np.random.RandomState(6)
    buf = rng.rand(m * lda + 1)
    A = buf[1:].reshape(m, lda)[:, :n]
    b = rng.rand(m) + 0.2
    x = rng.rand(n) / n + 1e-4
    fo, go = K.KLdiv(np.ascontiguousarray(A), b).func_grad(x, 2)
    bufd, bd, xd = dev(buf), dev(b), dev(x)
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    ax = torch.empty(m, dtype=torch.float64, device="cuda")
    h = C.c_void_p()
    assert lib.accbpg_kldiv_create(bufd.data_ptr() + 8, m, n, lda, bd.data_ptr(), None, C.byref(h)) == 0
    assert lib.accbpg_kldiv_set_stream(h, None) == 0
    fv = C.c_double()
    assert lib.accbpg_kldiv_func_grad(h, xd.data_ptr(), 2, C.byref(fv), g.data_ptr()) == 0
    assert lib.accbpg_kldiv_get_ax(h, ax.data_ptr()) == 0
    torch.cuda.synchronize()
    assert fv.value == pytest.approx(fo, rel=1e-13)
    np.testing.assert_allclose(g.cpu().numpy(), go, rtol=1e-12, atol=1e-13 * np.abs(go).max())
    np.testing.assert_allclose(ax.cpu().numpy(), np.ascontiguousarray(A) @ x, rtol=1e-13)
    assert lib.accbpg_kldiv_func_grad(h, xd.data_ptr(), 3, C.byref(fv), g.data_ptr()) == _lib.ERR_ARG
    assert lib.accbpg_kldiv_func_grad(h, xd.data_ptr(), 1, C.byref(fv), None) == _lib.ERR_ARG
    assert lib.accbpg_kldiv_create(bufd.data_ptr(), m, n, n - 1, bd.data_ptr(), None, C.byref(C.c_void_p())) \
        == _lib.ERR_ARG
    assert lib.accbpg_kldiv_destroy(h) == 0


# ------------------------------------------------------------------ assertions
def test_kl_and_shannon_assertions(acc):
    """functions.py:130, 142, 408, 413, 418, 428, 436-437, 483, 487-488; applications.py:199."""
    rng = np.random.RandomState(0)
    A, b = rng.rand(20, 30), rng.rand(20) + 0.1
    with pytest.raises(AssertionError, match="A and b size not matching"):
        acc.KLdivRegression(A, b[:-1])
    f = acc.KLdivRegression(A, b)
    with pytest.raises(AssertionError, match="NonnegRegression: x.size not equal to n."):
        f.func_grad(np.ones(29))
    with pytest.raises(AssertionError, match="need b > 0"):
        acc.KL_nonneg_regr(20, 30, noise=1e3, randseed=3)
    g = np.linspace(-0.5, 2.0, 30)
    y = np.full(30, 0.1)
    for h in (acc.ShannonEntropy(), acc.ShannonEntropyL1(0.25), acc.ShannonEntropySimplex()):
        with pytest.raises(AssertionError, match="require L > 0"):
            h.prox_map(g, 0.0)
        with pytest.raises(AssertionError):
            h.div_prox_map(y, g, -1.0)
        with pytest.raises(AssertionError):
            h.div_prox_map(y[:-1], g, 1.0)
        yn = y.copy()
        yn[17] = -1e-300
        with pytest.raises(AssertionError):
            h.div_prox_map(yn, g, 1.0)
        with pytest.raises(AssertionError, match="Some entries are negative."):
            h.divergence(yn, y)
        with pytest.raises(AssertionError, match="Some entries are negative."):
            h.divergence(y, yn)
        with pytest.raises(AssertionError):
            h.divergence(y[:-1], y)
        with pytest.raises(AssertionError, match="nonnegative"):
            h.gradient(yn)
    y0 = y.copy()
    y0[3] = 0.0
    np.testing.assert_allclose(acc.ShannonEntropy().div_prox_map(y0, g, 2.0), K.Shannon().div_prox_map(y0, g, 2.0),
                               rtol=1e-15)
    with pytest.raises(AssertionError, match="positive arguments"):
        acc.ShannonEntropySimplex().div_prox_map(y0, g, 2.0)    # strict y > 0 on the simplex (:488)
    h = acc.ShannonEntropy()
    yy = np.maximum(y0, 1e-20)
    assert h(y0) == pytest.approx(float(np.sum(yy * np.log(yy))), rel=1e-13)
    np.testing.assert_allclose(h.gradient(y0), 1.0 + np.log(yy), rtol=1e-15)


# ------------------------------------------------------------------ Shannon kernels over n
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 1025, 4097, 65537, 300000])
def test_shannon_kernels_over_n(acc, n):
    rng = np.random.RandomState(n)
    x = rng.rand(n)
    y = rng.rand(n) + 1e-3
    g = rng.randn(n)
    x[::3] = 0.0                                           # exact zeros: the delta path of the divergence
    y0 = y.copy()
    y0[1::4] = 0.0
    for _, hk, ho in _kernels(acc):
        for Lc in (0.7, 3.0):
            p = ho.prox_map(g, Lc)
            tol = 1e-15 if not isinstance(ho, K.ShannonSimplex) else 1e-15 + 2 * n * EPS
            np.testing.assert_allclose(hk.prox_map(g, Lc), p, rtol=tol)
            np.testing.assert_allclose(hk.div_prox_map(y, g, Lc), ho.div_prox_map(y, g, Lc), rtol=tol)
            if not isinstance(ho, K.ShannonSimplex):
                np.testing.assert_allclose(hk.div_prox_map(y0, g, Lc), ho.div_prox_map(y0, g, Lc), rtol=tol)
        for a, b in ((x, y), (y, x), (x, y0), (y0, y0)):
            terms = np.concatenate([a * np.log((a + 1e-20) / (b + 1e-20)), a, b])
            assert abs(hk.divergence(a, b) - ho.divergence(a, b)) <= _sum_tol(terms)


def test_shannon_ls_terms_fused(acc):
    """(<g,x-y>, D(x,y), D(z,z1)) in one pass: each term as the separate calls, with g and z optional."""
    from accbpg_and_fw_amd.functions import shannon_ls_terms, vec_dot_diff
    n = 4099
    rng = np.random.RandomState(2)
    g, x, y, z, z1 = (dev(rng.rand(n) + 0.01) for _ in range(5))
    h = acc.ShannonEntropy()
    lin, dxy, dzz = shannon_ls_terms(g, x, y, z, z1)
    assert lin == vec_dot_diff(g, x, y)
    assert dxy == h.divergence(x, y) and dzz == h.divergence(z, z1)
    lin0, dxy0, dzz0 = shannon_ls_terms(None, x, y)
    assert lin0 == 0.0 and dzz0 == 0.0 and dxy0 == dxy


# ------------------------------------------------------------------ the notebook's calls
def _six(acc, f, h, L, x0, N):
    return {
        "bpg": acc.BPG(f, h, L, x0, maxitrs=N, linesearch=False, verbose=False)[:3],
        "bpgls": acc.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.2, verbose=False)[:3],
        "abpg": acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=True, restart=False, verbose=False)[:3],
        "abpgrs": acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=True, restart=True, verbose=False)[:3],
        "gain": acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, theta_eq=True, restart=False,
                              verbose=False)[:3],
        "gainrs": acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, theta_eq=True, restart=True,
                                restart_rule='f', verbose=False)[:3]}


# G prefix that must agree to 1e-6: the length over which the reference keeps it under a change of summation
# order (238 / 107 for ABPG; whole runs otherwise), halved.  BPG-LS is the exception: with L_k cut by 1.2 per
# accepted step the iteration x <- x*exp(-(lamda+g)/L) amplifies rounding by ~1/L per step, and the reference itself,
# with its gradient formed by BLAS (np.dot(r, A)) instead of its column sums, leaves its own F at k = 16 / 17 (1e-12)
# and its own L_k sequence at k = 20 -- where the device run leaves it too; the runs meet again at the same F.
G_PREFIX = {"bpg": 2000, "bpgls": 19, "abpg": 50, "abpgrs": 45, "gain": 1000, "gainrs": 149}


@pytest.mark.parametrize("tag,m,n", SIZES)
def test_kl_notebook_trajectories(acc, tag, m, n):
    gd = golden("kl")
    f, h, L, x0 = acc.KL_nonneg_regr(m, n, **ARGS)
    for name, (x, F, G) in _six(acc, f, h, L, x0, 2000).items():
        Fr, Gr, xr = gd["%s_%s_F" % (tag, name)], gd["%s_%s_G" % (tag, name)], gd["%s_%s_x" % (tag, name)]
        k = min(len(F), len(Fr))
        assert _agree_prefix(G, Gr, 1e-6) >= min(G_PREFIX[name], k), name
        if name == "bpgls":
            assert _agree_prefix(F, Fr, 1e-12) >= 15
            assert len(F) == len(Fr) and abs(F[-1] - Fr[-1]) < 1e-6 * abs(Fr[-1])
            assert np.max(np.abs(x - xr)) < 1e-4
            continue
        # restart and stopping decisions of the restarted runs at (100,1000) are made at rounding level (the
        # reference's own length moves from 356 / 299 to 444 / 367 with the summation order): F on the common part
        _close(F[:k], Fr[:k], 1e-8)
        if len(F) == len(Fr):
            # to 1e-9 while the line-search decisions agree throughout, else where they meet again
            split = _agree_prefix(G, Gr, 1e-6) < k
            assert np.max(np.abs(x - xr)) < (1e-6 if split else 1e-9), name
        else:
            assert tag == "s2" and name in ("abpgrs", "gainrs"), name


@pytest.mark.parametrize("tag,m,n", SIZES)
def test_kl_notebook_printed_rows(acc, tag, m, n):
    """F at the printed rows k = 0, 1000, ..., 4000 of the 5000-iteration runs, to the printed digits."""
    gd = golden("kl")
    f, h, L, x0 = acc.KL_nonneg_regr(m, n, **ARGS)
    for name, (x, F, G) in _six(acc, f, h, L, x0, 5000).items():
        rows = gd["%s_%s_rows" % (tag, name)]
        for k, v in zip([0, 1000, 2000, 3000, 4000], rows):
            if np.isfinite(v) and k < len(F):
                assert "%.3e" % F[k] == "%.3e" % v, (name, k)


def test_kl_verbose_rows(acc, capsys):
    f, h, L, x0 = acc.KL_nonneg_regr(1000, 100, **ARGS)
    acc.BPG(f, h, L, x0, maxitrs=1001, linesearch=False, verbskip=1000)
    acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=1, theta_eq=True, verbskip=1000)
    acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=1, G0=0.1, theta_eq=True, verbskip=1000)
    lines = capsys.readouterr().out.split("\n")
    assert "BPG_LS method for min_{x in C} F(x) = f(x) + Psi(x)" in lines
    assert "     k      F(x)         Lk       time" in lines
    assert "ABPG method for minimize_{x in C} F(x) = f(x) + Psi(x)" in lines
    assert "ABPG_gain method for min_{x in C} F(x) = f(x) + Psi(x)" in lines
    rows = [ln for ln in lines if ln.startswith("     0 ") or ln.startswith("  1000 ")]
    # ex_KL_regr_L1.ipynb cell 3, the time column aside
    assert rows[0].startswith("     0   3.079e-01   1.000e+00 ") and rows[0].split()[:-1] == ["0", "3.079e-01", "1.000e+00"]
    assert rows[1].split()[:-1] == ["1000", "1.287e-01", "1.000e+00"]
    assert rows[2].startswith("     0   3.079e-01   1.000e+00   1.000e+00   1.470e-01   1.470e-01 ")
    assert rows[3].startswith("     0   3.079e-01   1.000e+00   1.070e+00   1.000e+00   1.280e-01   1.280e-01"
                              "   1.034e-01 ")


# ------------------------------------------------------------------ device tensors, large properties
def test_kl_device_tensors_stay_on_device(acc):
    f, h, L, x0 = acc.KL_nonneg_regr(300, 200, **ARGS)
    xd = dev(x0)
    fx, g = f.func_grad(xd, 2)
    assert isinstance(g, torch.Tensor) and g.is_cuda
    fn, gn = f.func_grad(x0, 2)
    assert fx == fn
    np.testing.assert_array_equal(g.cpu().numpy(), gn)
    for hk in (acc.ShannonEntropy(), acc.ShannonEntropyL1(0.01), acc.ShannonEntropySimplex()):
        for out in (hk.prox_map(g, 1.0), hk.div_prox_map(xd, g, 1.0)):
            assert isinstance(out, torch.Tensor) and out.is_cuda
        np.testing.assert_array_equal(hk.div_prox_map(xd, g, 1.0).cpu().numpy(), hk.div_prox_map(x0, gn, 1.0))
    x, F, G, T = acc.ABPG(f, h, L, xd, gamma=2.0, maxitrs=20, theta_eq=True, verbose=False)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    xn, Fn, Gn, Tn = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=20, theta_eq=True, verbose=False)
    np.testing.assert_array_equal(x.cpu().numpy(), xn)
    np.testing.assert_array_equal(F, Fn)


def test_kl_large_properties(acc):
    """(8192, 65536), 4 GiB of A: f(x*) = 0 and g(x*) = 0 at a consistent x* (b = the kernel's own A x*, so
    log(Ax/b) is exactly 0), directional derivative against a central difference, convexity along a segment."""
    m, n = 8192, 65536
    gen = torch.Generator(device="cuda").manual_seed(4)
    A = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=gen)
    xs = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) / n
    b0 = torch.ones(m, dtype=torch.float64, device="cuda")
    f0 = acc.KLdivRegression(A, b0)
    f0.func_grad(xs, 0)
    b = torch.from_numpy(f0.fitted()).cuda()
    del f0
    f = acc.KLdivRegression(A, b)
    fs, gs = f.func_grad(xs, 2)
    assert fs == 0.0 and float(gs.abs().max()) == 0.0
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) / n + 1e-6
    d = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * 1e-6
    fx, g = f.func_grad(x, 2)
    t = 1e-3
    num = (f(x + t * d) - f(x - t * d)) / (2 * t)
    assert float(g @ d) == pytest.approx(num, rel=1e-6)
    mid = f(0.5 * (x + xs))
    assert mid <= 0.5 * (fx + fs) + 1e-12 and fx > 0
    del A
