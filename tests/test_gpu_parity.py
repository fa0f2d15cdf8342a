"""GPU parity tests: the HIP path, called through the C-ABI, against the CPU oracle on the
same seeded inputs, against golden vectors written by the real reference, and -- at the
BASELINE sizes -- through size-independent properties."""
import ctypes as C

import numpy as np
import pytest

from conftest import golden, gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def O():
    from oracle import np_oracle
    return np_oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ MFMA engine
@pytest.mark.parametrize("config", [0, 1])
@pytest.mark.parametrize("kmajor", [0, 1])
@pytest.mark.parametrize("shape", [(64, 64, 64), (256, 128, 48), (300, 200, 77), (129, 65, 33),
                                   (512, 384, 1000), (17, 5, 3)])
def test_mfma_gemm_matches_numpy(acc, config, kmajor, shape):
    """v_mfma_f64_16x16x4_f64 tile engine: operand maps, LDS images, edge guards.
    Asymmetric random operands (a transposed result must fail)."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    M, N, K = shape
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    A = rng.randn(M, K)
    B = rng.randn(K, N) if kmajor else rng.randn(N, K)
    C0 = rng.randn(M, N)
    alpha, beta = -1.25, 0.5
    ref = alpha * (A @ (B if kmajor else B.T)) + beta * C0
    Ad, Bd, Cd = dev(A), dev(B), dev(C0)
    rc = lib.accbpg_test_gemm(Ad.data_ptr(), K, Bd.data_ptr(), B.shape[1], Cd.data_ptr(), N, M, N, K,
                              kmajor, alpha, beta, config, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    got = Cd.cpu().numpy()
    scale = np.abs(A) @ np.abs(B if kmajor else B.T) + np.abs(C0)
    assert np.max(np.abs(got - ref) / scale) < 1e-14       # fp64, tolerance ~ K*eps relative to |A||B|


# ------------------------------------------------------------------ objective
@pytest.mark.parametrize("tag", ["80x200", "128x1024", "200x2000", "512x8192"])
def test_func_grad_matches_reference_golden(acc, O, tag):
    gd = golden("percall_" + tag)
    m, n, seed = int(gd["m"]), int(gd["n"]), int(gd["seed"])
    f, h, L, x0 = acc.D_opt_design(m, n, randseed=seed)
    for xk, fk, gk in [("x", "f", "g"), (None, "f0", "g0")]:
        x = gd[xk] if xk else x0
        fx, g = f.func_grad(x, 2)
        # tolerance: |f| ~ 10..100 absolute 1e-11; gradient relative 1e-11 (fp64, different
        # factorisation (Cholesky vs LU) and summation order)
        assert abs(fx - float(gd[fk])) < 1e-11 * max(1.0, abs(float(gd[fk])))
        np.testing.assert_allclose(g, gd[gk], rtol=1e-11, atol=0)
        assert f(x) == fx                                   # flag 0 is the same factorisation
        np.testing.assert_array_equal(f.gradient(x), g)
    # device-tensor protocol returns device tensors
    fx2, g2 = f.func_grad(dev(gd["x"]), 2)
    assert isinstance(g2, torch.Tensor) and g2.is_cuda
    np.testing.assert_allclose(g2.cpu().numpy(), gd["g"], rtol=1e-11)


@pytest.mark.parametrize("shape", [(13, 506, 0), (80, 200, 10), (100, 1001, 4), (333, 777, 5),
                                   (768, 2048, 6), (1024, 4096, 8), (1000, 3000, 9), (1280, 2560, 11),
                                   (1024, 4112, 12), (2304, 4608, 13), (1536, 2080, 14), (4096, 8192, 15),
                                   (3072, 49152, 16), (2560, 16384, 17), (1792, 57344, 18), (4100, 8200, 19)])
def test_func_grad_matches_oracle_ragged_sizes(acc, O, shape):
    """Sizes that are not tile multiples (odd n, odd m, big tile with edges); interior sizes whose
    Gram tile list holds dual diagonal tiles (even / odd count of them, short and long K ranges per
    workgroup, workgroups that walk through several whole tiles, tile-aligned unit ranges) and one with an
    odd number of k-steps, where the list stays plain.  From m = 4033 on the Cholesky runs its two-level
    scheme (outer panels of eight block columns); (4100, 8200) ends it with a one-column panel of four rows."""
    m, n, seed = shape
    V = gaussian_design(m, n, seed + 100)
    rng = np.random.RandomState(seed)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    f = acc.DOptimalObj(V)
    fo = O.DOptOracle(V)
    fx, g = f.func_grad(x, 2)
    fr, gr = fo.func_grad(x, 2)
    assert abs(fx - fr) < 1e-11 * max(1.0, abs(fr))
    np.testing.assert_allclose(g, gr, rtol=1e-11, atol=0)


@pytest.mark.parametrize("shape", [(64, 256), (300, 900), (520, 1600), (1100, 3000), (2048, 4100)])
def test_two_level_cholesky_forced_at_small_sizes(acc, O, shape):
    """The two-level Cholesky (production path from 64 block columns on, outer panels of 8 block columns)
    switched on at sizes the oracle factors in no time: one block column, a lone ragged outer panel,
    8 + 1 block columns with a last one of 8 rows, 8 + 8 + 2, and a whole number of outer panels."""
    from accbpg_and_fw_amd import _lib
    m, n = shape
    V = gaussian_design(m, n, m + n)
    rng = np.random.RandomState(m)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    f = acc.DOptimalObj(V)
    assert _lib.load().accbpg_debug_chol_variant(f._h, 2048 | (1 << 12)) == 0      # threshold: 1 block column
    fx, g = f.func_grad(x, 2)
    fr, gr = O.DOptOracle(V).func_grad(x, 2)
    assert abs(fx - fr) < 1e-11 * max(1.0, abs(fr))
    np.testing.assert_allclose(g, gr, rtol=1e-11, atol=0)
    assert f(x) == fx                                                    # value-only path, same factorisation
    # a matrix that is not positive definite is still reported from inside an outer panel
    xz = np.zeros(n)
    xz[: m // 2] = 2.0 / m
    with pytest.raises(ValueError):
        f(xz)


def test_gram_unaligned_x_through_c_abi(acc, O):
    """An x that is only 8-byte aligned on an instance whose Gram tile list holds dual tiles (the
    direct-to-LDS kernel reads x in 16-byte pieces): the library stages an aligned copy."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n = 1024, 2048
    V = gaussian_design(m, n, 321)
    rng = np.random.RandomState(1)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    f = acc.DOptimalObj(V)
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    buf[1:] = dev(x)
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    fv = C.c_double()
    assert lib.accbpg_dopt_func_grad(f._h, buf.data_ptr() + 8, 2, C.byref(fv), g.data_ptr()) == 0
    torch.cuda.synchronize()
    fr, gr = O.DOptOracle(V).func_grad(x, 2)
    assert abs(fv.value - fr) < 1e-11 * abs(fr)
    np.testing.assert_allclose(g.cpu().numpy(), gr, rtol=1e-11)


@pytest.mark.parametrize("n,ld", [(65536, 65536), (131072, 131072), (65536, 196608)])
def test_long_rows_column_blocks_against_oracle(acc, O, n, ld):
    """Rows of 65536 columns or more: the Gram matrix is formed column block by column block of V (one launch per block of
    32768, every segment through a slab, the fix-up launches add the blocks up), and where consecutive rows lie a
    megabyte or more apart (leading dimension >= 131072) the launches read a copy of V stored block by block that the
    handle makes once.  All three cases against the oracle through the C-ABI: blocks only; blocks + copy; blocks + copy of
    a matrix that is a column range of a wider one (ldv > n).  The x handed in is only 8-byte aligned."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m = 768
    gen = torch.Generator(device="cuda").manual_seed(n + ld)
    wide = torch.randn(m, ld, dtype=torch.float64, device="cuda", generator=gen)
    V = wide[:, :n]
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    buf[1:] = x
    h = C.c_void_p()
    _lib.check(lib.accbpg_dopt_create(C.c_void_p(wide.data_ptr()), m, n, ld, None, C.byref(h), 0), "accbpg_dopt_create")
    try:
        g = torch.empty(n, dtype=torch.float64, device="cuda")
        fv = C.c_double()
        fr, gr = O.DOptOracle(V.cpu().numpy()).func_grad(x.cpu().numpy(), 2)
        for xp in (x.data_ptr(), buf.data_ptr() + 8):
            assert lib.accbpg_dopt_func_grad(h, C.c_void_p(xp), 2, C.byref(fv), C.c_void_p(g.data_ptr())) == 0
            torch.cuda.synchronize()
            assert abs(fv.value - fr) < 1e-11 * abs(fr)
            np.testing.assert_allclose(g.cpu().numpy(), gr, rtol=1e-10)
        f0 = C.c_double()
        assert lib.accbpg_dopt_func_grad(h, C.c_void_p(x.data_ptr()), 0, C.byref(f0), None) == 0
        assert f0.value == fv.value                             # the value-only evaluation: the same Gram matrix
    finally:
        lib.accbpg_dopt_destroy(h)


def test_func_grad_errors(acc):
    """AssertionError / ValueError behaviour of accbpg/functions.py:44-50."""
    f, h, L, x0 = acc.D_opt_design(8, 20, randseed=3)
    with pytest.raises(AssertionError):
        f.func_grad(-x0)
    with pytest.raises(AssertionError):
        f.func_grad(x0[:-1])
    z = np.zeros(20)
    z[:3] = 1.0 / 3                      # rank 3 < m: Gram matrix singular
    with pytest.raises(ValueError, match="HXHT is singular or not positive definite"):
        f.func_grad(z)
    with pytest.raises(AssertionError):
        acc.DOptimalObj(np.zeros((5, 5)))


# ------------------------------------------------------------------ Burg kernel
@pytest.mark.parametrize("tag", ["80x200", "128x1024", "200x2000", "512x8192"])
def test_prox_and_divergence_match_reference_golden(acc, tag):
    gd = golden("percall_" + tag)
    h = acc.BurgEntropySimplex()
    for idx in range(3):
        z = h.div_prox_map(gd["y"], gd["g"], float(gd["prox_L%d" % idx]))
        # same scalar algorithm; only the reduction order of the two sums differs
        np.testing.assert_allclose(z, gd["prox_x%d" % idx], rtol=1e-12, atol=0)
        assert abs(z.sum() - 1) <= 1.001e-8               # stops at |phi| <= eps, not renormalised
    gg = gd["g"] - gd["g"].min() + 0.5
    np.testing.assert_allclose(h.prox_map(gg, 2.0), gd["prox_raw"], rtol=1e-12)
    assert h.divergence(gd["x"], gd["y"]) == pytest.approx(float(gd["div_xy"]), rel=1e-12)
    assert h.divergence(gd["y"], gd["x"]) == pytest.approx(float(gd["div_yx"]), rel=1e-12)
    assert h.extra_Psi(gd["x"]) == 0


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2048, 2049, 8193, 40000, 300000])
def test_prox_sizes_against_oracle(acc, O, n):
    """Every register-cached variant and burg_prox_multi_kernel<8> (n = 40000, 300000), ragged n.  The wide
    multi-workgroup form and the re-read variant start above n = 1048576 and 4194304: test_gpu_prox.py runs them."""
    rng = np.random.RandomState(n)
    y = rng.rand(n) + 1e-3
    y /= y.sum()
    g = -rng.rand(n) * 50 - 1
    h, ho = acc.BurgEntropySimplex(), O.BurgSimplexOracle()
    for L in (1.0, 0.02):
        z = h.div_prox_map(y, g, L)
        zo = ho.div_prox_map(y, g, L)
        np.testing.assert_allclose(z, zo, rtol=1e-11, atol=0)
        assert h.last_info[1] == ho.last_newton_steps


def test_burg_errors(acc):
    h = acc.BurgEntropySimplex()
    x = np.ones(10) / 10
    with pytest.raises(AssertionError):
        h.div_prox_map(x, x, -1.0)
    with pytest.raises(AssertionError):
        h.div_prox_map(0 * x, x, 1.0)
    with pytest.raises(AssertionError):
        h.divergence(x, 0 * x)
    with pytest.raises(AssertionError):
        h.divergence(x, x[:-1])


def test_vector_helpers(acc):
    from accbpg_and_fw_amd.functions import vec_axpby, vec_dot_diff, ls_terms, vec_min_sum
    rng = np.random.RandomState(5)
    n = 5003
    x, z, g = rng.rand(n) + .1, rng.rand(n) + .1, rng.randn(n)
    th = 0.3217
    out = vec_axpby(1 - th, dev(x), th, dev(z)).cpu().numpy()
    np.testing.assert_array_equal(out, (1 - th) * x + th * z)            # bitwise: no FMA contraction
    assert vec_dot_diff(dev(g), dev(x), dev(z)) == pytest.approx(np.dot(g, x - z), rel=1e-12)
    d, dxy, dzz = ls_terms(dev(g), dev(x), dev(z), dev(z), dev(x))
    assert dxy == pytest.approx(np.sum(x / z - np.log(x / z) - 1), rel=1e-12)
    assert dzz == pytest.approx(np.sum(z / x - np.log(z / x) - 1), rel=1e-12)
    mn, sm = vec_min_sum(dev(x))
    assert mn == x.min() and sm == pytest.approx(x.sum(), rel=1e-13)


# ------------------------------------------------------------------ solver trajectories
def _close(a, b, tol):
    assert a.shape == b.shape, (a.shape, b.shape)
    np.testing.assert_allclose(a, b, rtol=tol, atol=tol)


def _agree_prefix(a, b, tol):
    """length of the common prefix on which two traces agree to tol"""
    n = min(len(a), len(b))
    bad = np.nonzero(np.abs(a[:n] - b[:n]) > tol * (1 + np.abs(b[:n])))[0]
    return n if bad.size == 0 else int(bad[0])


def test_bpg_abpg_trajectories_80x200(acc):
    """1000 iterations at the notebook instance D_opt_design(80,200,randseed=10) with the notebook's
    calls (ipynb/ex_Dopt_random.ipynb cells 1 and 3): iterates within the north-star tolerance
    l_inf < 1e-9, traces to 1e-9, stored stdout rows reproduced."""
    gd = golden("traces_80x200")
    f, h, L, x0 = acc.D_opt_design(80, 200, randseed=10)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=1000, linesearch=False, verbose=False)
    assert np.max(np.abs(x - gd["bpg_x"])) < 1e-9
    _close(F, gd["bpg_F"], 1e-9)
    assert "%.3e" % F[0] == "1.910e+01" and "%.3e" % F[900] == "1.759e+01"   # ex_Dopt_random.ipynb:73,82
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=1000, linesearch=True, verbose=False)
    assert np.max(np.abs(x - gd["bpgls_x"])) < 1e-9
    _close(F, gd["bpgls_F"], 1e-9); _close(Ls, gd["bpgls_Ls"], 1e-12)
    assert "%.3e" % Ls[0] == "8.333e-01" and "%.3e" % Ls[100] == "1.938e-01"   # :243-244
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=1000, theta_eq=True, verbose=False)
    assert np.max(np.abs(x - gd["abpg_x"])) < 1e-9
    _close(F, gd["abpg_F"], 1e-9); _close(G[:500], gd["abpg_G"][:500], 1e-6)
    assert "%.3e" % G[100] == "5.529e-01"                                    # :113
    assert len(T) == len(F) and np.all(np.diff(T) >= 0)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=1000, theta_eq=True, restart=True, verbose=False)
    assert np.max(np.abs(x - gd["abpgrs_x"])) < 1e-9
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=1.5, maxitrs=1000, theta_eq=False, verbose=False)
    assert np.max(np.abs(x - gd["abpgk_x"])) < 1e-9
    _close(F, gd["abpgk_F"], 1e-9)


_GAIN_VARIANTS = [("gain", dict(G0=0.1, theta_eq=True)),
                  ("gainrs", dict(G0=0.1, theta_eq=True, restart=True)),
                  ("gaindef", dict()),
                  ("gainopt", dict(G0=0.1, ls_inc=1.5, ls_dec=1.1, theta_eq=False, checkdiv=True,
                                   restart=True, restart_rule='f'))]


def _check_gain_runs(acc, tag, stable, tol_x):
    """ABPG_gain takes discrete line-search decisions; once converged they sit at the rounding floor
    and the reference itself is not reproducible across BLAS thread counts (first differs at k=756 on
    (80,200), k=36..79 on (256,4096); tests/test_oracle.py).  So: identical gain sequence and F on the
    decision-stable prefix (>= `stable` iterations), objective-level agreement at the end."""
    gd = golden("traces_" + tag)
    m, n, seed, iters = int(gd["m"]), int(gd["n"]), int(gd["seed"]), int(gd["iters"])
    f, h, L, x0 = acc.D_opt_design(m, n, randseed=seed)
    for key, kw in _GAIN_VARIANTS:
        x, F, Gain, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=iters, verbose=False, **kw)
        ref_gain = gd[key + "_Gain"]
        k = _agree_prefix(Gain, ref_gain, 1e-12)
        assert k >= min(stable, len(ref_gain) - 5), (key, k)
        ks = min(k, stable)
        _close(F[:ks], gd[key + "_F"][:ks], 1e-9)           # decision-stable prefix: tight
        _close(F[:k], gd[key + "_F"][:k], 1e-5)             # same decisions, rounding already amplified
        _close(Gavg[:k], gd[key + "_Gavg"][:k], 1e-9)
        assert len(F) == len(Gain) == len(Gdiv) == len(Gavg) == len(T)
        nf = min(len(F), len(gd[key + "_F"]))
        # after the decisions part ways only the objective level is comparable (the reference itself
        # ends 1.5e-5 apart between 1 and 8 BLAS threads on (256,4096))
        assert abs(F[nf - 1] - gd[key + "_F"][nf - 1]) < 1e-4
        if k == len(ref_gain) == len(Gain):
            assert np.max(np.abs(x - gd[key + "_x"])) < tol_x
    return f, h, L, x0


def test_abpg_gain_trajectories_80x200(acc):
    f, h, L, x0 = _check_gain_runs(acc, "80x200", stable=400, tol_x=1e-9)
    x, F, Gain, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=200, G0=0.1, theta_eq=True,
                                               verbose=False)
    assert "%.3e" % Gain[0] == "2.488e-01" and "%.3e" % Gavg[0] == "4.988e-02"      # ex_Dopt_random.ipynb:282
    assert "%.3e" % Gain[100] == "2.986e-01" and "%.3e" % Gdiv[100] == "7.091e-01"  # :283


def test_early_stop_and_truncation_80x120(acc):
    """Stopping rules and array truncation (algorithms.py:66-71,174-179,412-419).  The stop tests
    compare rounding-level quantities with 1e-14, so the stopping iteration may move by a few
    iterations between summation orders; the traces must agree on the common prefix."""
    gd = golden("traces_80x120")
    f, h, L, x0 = acc.D_opt_design(80, 120, randseed=10)
    assert "%.3e" % f(x0) == "3.764e+01"                              # ex_Dopt_random.ipynb:398
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=300, linesearch=False, verbose=False)
    assert len(F) < 300 and len(F) == len(Ls) == len(T)
    n = min(len(F), len(gd["bpg_F"]))
    assert n >= 40
    _close(F[:n], gd["bpg_F"][:n], 1e-10)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=300, theta_eq=True, verbose=False)
    n = min(len(F), len(gd["abpg_F"]))
    assert len(F) < 300 and n >= 40
    _close(F[:n], gd["abpg_F"][:n], 1e-10)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=300, theta_eq=True, restart=True, verbose=False)
    n = min(len(F), len(gd["abpgrs_F"]))
    assert n >= 20
    _close(F[:n], gd["abpgrs_F"][:n], 1e-10)
    _check_gain_runs(acc, "80x120", stable=15, tol_x=1e-8)
    x, F, Gain, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=50, G0=0.1, theta_eq=True,
                                               verbose=False)
    assert "%.3e" % Gain[0] == "5.160e-01" and "%.3e" % Gavg[0] == "7.183e-02"      # ex_Dopt_random.ipynb:398-418


def test_trajectories_256x4096(acc):
    """1000-iteration l_inf parity at a size where the CPU side is affordable."""
    gd = golden("traces_256x4096")
    f, h, L, x0 = acc.D_opt_design(256, 4096, randseed=10)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=1000, linesearch=False, verbose=False)
    assert np.max(np.abs(x - gd["bpg_x"])) < 1e-9
    _close(F, gd["bpg_F"], 1e-9)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=1000, linesearch=True, verbose=False)
    assert np.max(np.abs(x - gd["bpgls_x"])) < 1e-9
    _close(Ls, gd["bpgls_Ls"], 1e-12)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=1000, theta_eq=True, verbose=False)
    assert np.max(np.abs(x - gd["abpg_x"])) < 1e-9
    _close(F, gd["abpg_F"], 1e-9)
    _check_gain_runs(acc, "256x4096", stable=30, tol_x=1e-9)


def test_reference_loop_runs_on_device_objects(acc, O):
    """Drop-in direction 2: a NumPy driver loop (here the oracle's BPG, which has the reference's
    structure) runs unchanged on this package's f / h objects."""
    gd = golden("traces_80x200")
    f, h, L, x0 = acc.D_opt_design(80, 200, randseed=10)
    x, F, Ls, T = O.BPG(f, h, L, x0, maxitrs=50, linesearch=False)
    _close(F, gd["bpg_F"][:50], 1e-10)


def test_housing_rng_free(acc):
    gd = golden("housing")
    V = gd["V"]
    n = V.shape[1]
    f, h = acc.DOptimalObj(V), acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    assert "%.3e" % f(x0) == "-4.137e+01"                             # ex_Dopt_LIBSVM.ipynb:191
    x, F, Ls, T = acc.BPG(f, h, 1.0, x0, maxitrs=1001, linesearch=False, verbose=False)
    _close(F, gd["bpg_F"], 1e-9)
    assert np.max(np.abs(x - gd["bpg_x"])) < 1e-9
    x, F, G, T = acc.ABPG(f, h, 1.0, x0, gamma=2, maxitrs=1001, verbose=False)
    _close(F, gd["abpg_F"], 1e-9)
    assert np.max(np.abs(x - gd["abpg_x"])) < 1e-9


# ------------------------------------------------------------------ Frank-Wolfe
@pytest.mark.parametrize("tag", ["30x1000", "64x512", "256x4096"])
def test_fw_trajectories(acc, tag):
    gd = golden("fw_" + tag)
    m, n, seed, iters = int(gd["m"]), int(gd["n"]), int(gd["seed"]), int(gd["iters"])
    V = gaussian_design(m, n, seed)
    x0 = np.ones(n) / n
    x, F, SP, SN, T = acc.D_opt_FW(V, x0, float(gd["eps"]), iters, verbose=False)
    assert len(F) == len(gd["fw_F"])
    assert np.max(np.abs(x - gd["fw_x"])) < 1e-9
    _close(F, gd["fw_F"], 1e-9); _close(SP, gd["fw_SP"], 1e-9); _close(SN, gd["fw_SN"], 1e-9)
    x, F, SP, SN, T = acc.D_opt_FW_away(V, x0, float(gd["eps"]), iters, verbose=False)
    assert abs(len(F) - len(gd["away_F"])) <= 2
    k = min(len(F), len(gd["away_F"]))
    assert np.max(np.abs(x - gd["away_x"])) < 1e-8
    _close(F[:k], gd["away_F"][:k], 1e-9); _close(SP[:k], gd["away_SP"][:k], 1e-8)
    # extension: determinant-lemma tracking of log det(H) between refactorisations
    x2, F2, SP2, SN2, T2 = acc.D_opt_FW_away(V, x0, float(gd["eps"]), iters, verbose=False, logdet_refresh=50)
    np.testing.assert_array_equal(x2, x)
    _close(F2[:k], F[:k], 1e-9)


@pytest.mark.parametrize("shape", [(64, 512), (256, 4096), (1536, 4096)])
def test_fw_away_logdet_forms_agree(acc, O, shape):
    """F[k] = log det(H_k) of D_opt_FW_away (accbpg/D_opt_alg.py:136) is a logged value; the forms it can be produced in
    -- a fresh factorisation every iteration with 1 or 3 of them in flight beside the steps, anchored every R-th
    iteration with log-space steps in between (the default, R = 16), never refactored -- leave iterates, gaps and step
    choices BIT-identical, give the identical F where every iteration is factored, and F within 1e-12 (1 + |F|) of that
    otherwise; and all of them follow the oracle's trace."""
    m, n = shape
    V = gaussian_design(m, n, 19)
    x0 = np.ones(n) / n
    iters = 300
    f = acc.DOptimalObj(V)
    ref = acc.D_opt_FW_away(f, x0, -1.0, iters, verbose=False, logdet_refresh=1, logdet_ring=1)
    xo, Fo, SPo, SNo, To = O.D_opt_FW_away(V, x0, -1.0, iters)
    _close(ref[1], Fo, 1e-9); _close(ref[2], SPo, 1e-7)
    assert np.max(np.abs(ref[0] - xo)) < 1e-10
    for kw in (dict(logdet_refresh=1, logdet_ring=3), dict(logdet_refresh=1, logdet_ring=2), dict(), dict(logdet_refresh=16),
               dict(logdet_refresh=7), dict(logdet_refresh=64), dict(logdet_refresh=1000), dict(logdet_refresh=0)):
        x, F, SP, SN, T = acc.D_opt_FW_away(f, x0, -1.0, iters, verbose=False, **kw)
        np.testing.assert_array_equal(x, ref[0])
        np.testing.assert_array_equal(SP, ref[2])
        np.testing.assert_array_equal(SN, ref[3])
        assert len(F) == iters
        if kw.get("logdet_refresh") == 1:
            np.testing.assert_array_equal(F, ref[1])
        else:
            assert np.max(np.abs(F - ref[1]) / (1 + np.abs(ref[1]))) < 1e-12, kw
    # an evaluation on the same handle while factorisations are in flight, and a run that ends early
    from accbpg_and_fw_amd.D_opt_alg import D_opt_FW_away_steps
    gen = D_opt_FW_away_steps(f, x0, -1.0, 50, verbose=False, logdet_refresh=1, logdet_ring=3)
    for _ in range(10):
        next(gen)
    fv, g = f.func_grad(x0, 2)                                   # while three factorisations are in flight
    fo, go = O.DOptOracle(V).func_grad(x0, 2)
    assert abs(fv - fo) < 1e-11 * max(1.0, abs(fo))
    np.testing.assert_allclose(g, go, rtol=1e-10)
    gen.close()                                                  # abandoned with factorisations in flight
    again = acc.D_opt_FW_away(f, x0, -1.0, iters, verbose=False, logdet_refresh=1, logdet_ring=1)
    np.testing.assert_array_equal(again[1], ref[1])
    # the stopping rule ends a run where the reference's does (eps large enough to be met)
    if m <= 64:
        xs, Fs, SPs, SNs, Ts = acc.D_opt_FW_away(f, x0, 0.3, 3000, verbose=False)
        xr, Fr, SPr, SNr, Tr = O.D_opt_FW_away(V, x0, 0.3, 3000)
        assert len(Fs) == len(Fr) and 1 < len(Fs) < 3000
        _close(Fs, Fr, 1e-9)


def test_fw_housing_and_state(acc):
    gd = golden("housing")
    V = gd["V"]
    n = V.shape[1]
    x0 = np.ones(n) / n
    x, F, SP, SN, T = acc.D_opt_FW_away(V, x0, 1e-8, 3000, verbose=False)
    k = min(len(F), len(gd["away_F"]))
    _close(F[:k], gd["away_F"][:k], 1e-8)
    assert np.max(np.abs(x - gd["away_x"])) < 1e-8
    assert abs(x.sum() - 1) < 1e-9 and x.min() > -1e-15


# ------------------------------------------------------------------ BASELINE size (config 2 / 3)
@pytest.fixture(scope="module")
def large(acc):
    gd = golden("large_percall")
    f, h, L, x0 = acc.D_opt_design(int(gd["m"]), int(gd["n"]), randseed=int(gd["seed"]))
    return f, h, L, x0, gd


def test_large_percall_2048x32768(large):
    """Per-call parity at D_opt_design(2048,32768): f, g, prox, divergence against values the real
    reference produced for the same seed (oracle/gen_golden.py --large)."""
    f, h, L, x0, gd = large
    f0, g0 = f.func_grad(x0, 2)
    assert abs(f0 - float(gd["f0"])) < 1e-10 * abs(float(gd["f0"]))
    np.testing.assert_allclose(g0, gd["g0"], rtol=1e-11)
    fx, g = f.func_grad(gd["x"], 2)
    assert abs(fx - float(gd["f"])) < 1e-10 * abs(float(gd["f"]))
    np.testing.assert_allclose(g, gd["g"], rtol=1e-11)
    z = h.div_prox_map(gd["x"], gd["g"], 1.0)
    np.testing.assert_allclose(z, gd["prox"], rtol=1e-11)
    assert h.divergence(gd["prox"], gd["x"]) == pytest.approx(float(gd["div"]), rel=1e-11)


def test_large_properties_2048x32768(large):
    """Size-independent properties: sum_i x_i * (-g_i) = m (trace identity of the D-optimal
    gradient), f(c*x) = f(x) - m*log(c), gradient is (-1)-homogeneous."""
    f, h, L, x0, gd = large
    m = f.m
    x = gd["x"]
    fx, g = f.func_grad(x, 2)
    assert abs(np.dot(x, -g) - m) < 1e-9 * m
    c = 1.7
    f2, g2 = f.func_grad(c * x, 2)
    assert abs(f2 - (fx - m * np.log(c))) < 1e-9 * abs(fx)
    np.testing.assert_allclose(g2 * c, g, rtol=1e-11)
    z = h.div_prox_map(x, g, 1.0)
    assert z.min() > 0 and abs(z.sum() - 1) <= 1.001e-8
    assert h.divergence(x, x) == 0.0


def test_large_abpg_gain_trajectory_2048x32768(large, acc):
    """12 iterations of ABPG_gain(gamma=2) at config 2 against the real reference's trace."""
    f, h, L, x0, _ = large
    gd = golden("large_gain")
    iters = int(gd["iters"])
    x, F, Gain, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=iters, verbose=False)
    assert np.max(np.abs(x - gd["x"])) < 1e-9
    _close(F, gd["F"], 1e-9); _close(Gain, gd["Gain"], 1e-12); _close(Gdiv, gd["Gdiv"], 1e-7)


class _LoggedObjective:
    """Pass-through over a DOptimalObj that notes kind, returned value and (at the call positions in `tap_positions`)
    the argument of every oracle call, in the order the reference's loop makes them (the way oracle/gen_golden.py's
    _CallLog notes the reference's).  overlap=False puts F[k] = f(x) on the solver's stream; overlap=True is the
    package default: the solvers start F[k] through value_async on the objective's second handle and stream (whose
    factorisation runs in small launches for m > 1408) beside func_grad(y) and collect it through value_wait -- the
    value is logged at the position of the call that started it, which is where the reference evaluates it."""

    def __init__(self, f, overlap, tap_positions=()):
        self.f = f
        self.m, self.n, self.H = f.m, f.n, f.H
        self.device = f.device
        self._overlap = bool(overlap)
        self._lin = False
        self.kinds, self.values, self.taps = [], [], {}
        self.async_values = 0
        self.tap_positions = set(int(p) for p in tap_positions)

    def _note(self, x):
        if len(self.kinds) in self.tap_positions:
            self.taps[len(self.kinds)] = x.detach().clone()

    def __call__(self, x):
        self._note(x)
        v = self.f.func_grad(x, 0)
        self.kinds.append(0); self.values.append(v)
        return v

    def value_async(self, x):
        self._note(x)
        self.kinds.append(0); self.values.append(float("nan"))
        self.async_values += 1
        return (len(self.values) - 1, self.f.value_async(x))

    def value_wait(self, ticket):
        pos, inner = ticket
        v = self.f.value_wait(inner)
        self.values[pos] = v
        return v

    def value_lead_seconds(self):
        return self.f.value_lead_seconds()

    def func_grad(self, x, flag=2):
        self._note(x)
        out = self.f.func_grad(x, flag)
        self.kinds.append(flag); self.values.append(out[0] if flag == 2 else float("nan"))
        return out

    def gradient(self, x):
        return self.func_grad(x, 1)


@pytest.mark.parametrize("overlap", [False, True])
def test_large_abpg_gain_past_first_retries_2048x32768(large, acc, overlap):
    """The headline solver at the headline size through the first line-search retries: 64 iterations of
    ABPG_gain(gamma=2) at D_opt_design(2048,32768) against the trace of the real reference
    (oracle/gen_golden.py --only-large-gain-long; accbpg/algorithms.py:361-390).  The fixture holds the
    gain sequence, the value EVERY oracle call returned in call order (rejected trial points included), and
    iterates x_k along the run.  Required: the same accept/reject decisions (identical gain sequence and call
    pattern), every F[k] to 1e-9 (every evaluated objective value, rejected trial points too, to 1e-7),
    l_inf(x_k) < 1e-9 at the stored iterates.  Run on both evaluation paths: F[k] on the solver's stream, and the package
    default (F[k] on the second handle and stream beside func_grad(y), its factorisation in small launches)."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "large_gain_long.npz")):
        pytest.skip("tests/golden/large_gain_long.npz not generated")
    f, h, L, x0, _ = large
    gd = golden("large_gain_long")
    iters = int(gd["iters"])
    ref_gain = gd["Gain"]
    retries = np.flatnonzero(ref_gain[1:] > ref_gain[:-1] / 1.2 * (1 + 1e-12)) + 1
    assert retries.size >= 10, "fixture must contain line-search retries"     # the regime the solver lives in

    keep = set(int(k) for k in gd["keep"])
    from accbpg_and_fw_amd.algorithms import ABPG_gain_steps
    xd = torch.from_numpy(x0).cuda()
    logged = _LoggedObjective(f, overlap)
    gen = ABPG_gain_steps(logged, h, L, xd, 2, iters, verbose=False)
    result = None
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            result = stop.value
            break
    kinds, values = logged.kinds, logged.values
    assert logged.async_values == (iters if overlap else 0)     # overlap=True really ran F[k] on the side handle
    x, F, Gain, Gdiv, Gavg, T = result
    assert len(F) == iters
    np.testing.assert_array_equal(np.array(kinds, dtype=np.int8), gd["call_kinds"])     # same call pattern
    _close(Gain, ref_gain, 1e-12)                                                       # same decisions
    # every evaluated value, rejected trial points included: those lie a too-long step away, where the objective
    # is less well conditioned than along the iterates (measured: one of the 280 values off by 9e-9 relative, the
    # others and every F[k] below 1e-9)
    _close(np.array(values), gd["call_values"], 1e-7)
    assert np.sum(np.abs(np.array(values) - gd["call_values"]) > 1e-9 * (1 + np.abs(gd["call_values"]))) <= 3
    _close(F, gd["F"], 1e-9); _close(Gavg, gd["Gavg"], 1e-11)
    # Gdiv = D(x+,y) / D(z+,z) / theta^gamma is a ratio of two divergences whose terms r - log r - 1 cancel to
    # ~(r-1)^2/2: each carries a relative rounding error of about eps/(r-1)^2, so the ratio is known to ~1e-4 only
    # (measured 3e-5; it is a diagnostic column, no decision reads it unless checkdiv is set)
    _close(Gdiv, gd["Gdiv"], 1e-3)
    assert np.max(np.abs(x.cpu().numpy() - gd["x"])) < 1e-9
    # iterates along the run: rerun to each stored k (the solver is deterministic) -- the shortest prefixes only
    for k in sorted(keep)[:3]:
        xk = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=k, verbose=False)[0]
        assert np.max(np.abs(xk - gd["x_%d" % k])) < 1e-9, k
    # the mix in the retry regime: about 2 gradient and 3 value evaluations per iteration
    pos = gd["iter_call_pos"]
    tail = slice(int(pos[40]), int(pos[60]))
    kk = np.array(kinds)[tail]
    assert 1.7 <= np.sum(kk == 2) / 20 <= 2.3 and 2.6 <= np.sum(kk == 0) / 20 <= 3.4


def _logged_gain_run(f, h, L, x0, iters, tap_positions=(), overlap=False):
    """ABPG_gain(gamma=2) with kind, returned value and (at the call positions in `tap_positions`) the argument of
    every oracle call noted (_LoggedObjective)."""
    logged = _LoggedObjective(f, overlap, tap_positions)
    from accbpg_and_fw_amd.algorithms import ABPG_gain_steps
    gen = ABPG_gain_steps(logged, h, L, torch.from_numpy(x0).cuda(), 2, iters, verbose=False)
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            assert logged.async_values == (iters if overlap else 0)
            return stop.value, np.array(logged.kinds, dtype=np.int8), np.array(logged.values), logged.taps


@pytest.mark.parametrize("overlap", [False, True])
def test_large_abpg_gain_300_iterations_2048x32768(large, acc, overlap):
    """The headline solver at the headline size deep into the regime it lives in: 300 iterations of ABPG_gain(gamma=2)
    at D_opt_design(2048,32768) against the call log of the real reference (oracle/gen_golden.py
    --only-large-gain-long --iters 300 --name large_gain_300; 2.1 hours of CPU; accbpg/algorithms.py:295-420): 1458
    oracle calls, about 2 gradient + 3 value evaluations per iteration from k = 30 on.

    ABPG_gain's accept/reject test compares two nearly equal numbers, and the reference's own outcome flips with the
    BLAS thread count once a comparison falls inside rounding: at THIS size the real reference run with 4 instead of
    8 OpenBLAS threads makes a different decision at k = 86 (oracle call 391), its F[k] is off by more than 1e-9 from
    k = 84 and its x_100 by 4.7e-7 (profiles/r02_reference_self_spread.json, tools/reference_self_spread.py).  The
    HIP path stays closer to the 8-thread reference than that.  So the requirement is stated on the
    decision-stable prefix [0, stable): identical call pattern (every accept/reject decision), identical gain
    sequence, every F[k] to 1e-9 while the run is young and to 1e-8 up to the end of the prefix, and the iterate the
    prefix ends in to l_inf < 1e-8.  Measured: stable = 100 iterations = 456 oracle calls, 78 of them retries;
    max relative gap of F[k] 6.8e-9 (around k = 78; below 1e-9 for k < 78 and again from k = 85); l_inf(x_100) = 3.7e-9.  Rejected trial points
    lie a too-long step away, close to where the Gram matrix loses rank, and their values are far more sensitive
    (one of the 178 differs by 1.5e-5 relative): they only have to agree to 1e-4.  Beyond the prefix both runs are valid
    ABPG_gain runs of the same instance that took different branches: their objective values must stay together
    (measured: within 5e-6 relative throughout, 7e-7 at k = 299)."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "large_gain_300.npz")):
        pytest.skip("tests/golden/large_gain_300.npz not generated")
    f, h, L, x0, _ = large
    gd = golden("large_gain_300")
    iters = int(gd["iters"])
    pos = gd["iter_call_pos"]
    ref_gain = gd["Gain"]
    ref_kinds, ref_values = gd["call_kinds"], gd["call_values"]
    keep = [int(k) for k in gd["keep"]]
    (x, F, Gain, Gdiv, Gavg, T), kinds, values, taps = _logged_gain_run(f, h, L, x0, iters, [pos[k] for k in keep], overlap)
    assert len(F) == iters
    differs = np.flatnonzero(np.abs(Gain - ref_gain) > 1e-12 * np.abs(ref_gain))
    stable = int(differs[0]) if differs.size else iters           # iterations [0, stable) made the same decisions
    relF = np.abs(F - gd["F"]) / (1 + np.abs(gd["F"]))
    print("decision-stable prefix: %d of %d iterations; max rel gap of F on it %.2e, beyond it %.2e"
          % (stable, iters, relF[:stable].max(), relF.max()))
    assert stable >= 90                                            # measured: 100
    ncalls = int(pos[stable]) if stable < iters else len(ref_kinds)
    np.testing.assert_array_equal(kinds[:ncalls], ref_kinds[:ncalls])
    assert int(np.sum(ref_kinds[:ncalls] == 2)) - stable >= 60     # the prefix is in the retry regime (78 retries)
    young = min(stable, 70)
    assert relF[:young].max() < 1e-9
    assert relF[:stable].max() < 1e-8
    _close(Gavg[:stable], gd["Gavg"][:stable], 1e-11)
    # every evaluated value on the prefix: the accepted ones are F[k]; the rejected trial values are looser (docstring)
    have = ~np.isnan(ref_values[:ncalls])
    relv = np.abs(values[:ncalls][have] - ref_values[:ncalls][have]) / (1 + np.abs(ref_values[:ncalls][have]))
    assert relv.max() < 1e-4 and np.mean(relv > 1e-8) < 0.05
    # the iterate the prefix ends in (and any stored one inside it)
    for k in keep:
        if k <= stable and int(pos[k]) in taps:
            gap = np.max(np.abs(taps[int(pos[k])].cpu().numpy() - gd["x_%d" % k]))
            print("l_inf(x_%d) = %.2e" % (k, gap))
            assert gap < 1e-8, k
    assert any(k <= stable for k in keep)
    # beyond the prefix: the same objective values, by a margin that says "same minimisation", not "same branch"
    assert relF.max() < 5e-5
    assert abs(F[-1] - gd["F"][-1]) < 1e-5 * abs(gd["F"][-1])
    # and the run is a descent run in its own right
    assert np.all(np.diff(F) < 1e-9 * np.abs(F[:-1]))


@pytest.mark.parametrize("overlap", [False, True])
def test_large_abpg_1000_iterations_2048x32768(large, acc, overlap):
    """The north-star horizon at the headline size: 1000 iterations of ABPG(gamma=2, theta_eq=True) at
    D_opt_design(2048,32768) against the real reference (oracle/gen_golden.py --only-large-abpg-1000, about three hours
    of CPU; accbpg/algorithms.py:118-193).  l_inf(x_k) < 1e-9 at k = 250, 500, 750 and 1000, every F[k] to 1e-9.  Run on both
    evaluation paths: F[k] on the solver's stream, and the package default (F[k] on the second handle and stream beside
    the gradient evaluation, its factorisation in small launches)."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "large_abpg_1000.npz")):
        pytest.skip("tests/golden/large_abpg_1000.npz not generated")
    f, h, L, x0, _ = large
    gd = golden("large_abpg_1000")
    iters = int(gd["iters"])
    keep = sorted(int(k) for k in gd["keep"])
    # the argument of value call k = the iterate x_k (accbpg/algorithms.py:135): one value and one gradient
    # evaluation per iteration, so it is oracle call 2k
    tap = _LoggedObjective(f, overlap, [2 * k for k in keep])
    from accbpg_and_fw_amd.algorithms import ABPG
    x, F, G, T = ABPG(tap, h, L, torch.from_numpy(x0).cuda(), gamma=2.0, maxitrs=iters, theta_eq=True, verbose=False)
    assert tap.async_values == (iters if overlap else 0)
    kept = {k: tap.taps[2 * k] for k in keep}
    x = x.cpu().numpy() if isinstance(x, torch.Tensor) else x
    assert len(F) == iters
    gaps = {k: float(np.max(np.abs(kept[k].cpu().numpy() - gd["x_%d" % k]))) for k in keep}
    gaps[iters] = float(np.max(np.abs(x - gd["x"])))
    print("l_inf(x_k):", gaps, " max rel gap of F: %.2e" % np.max(np.abs(F - gd["F"]) / (1 + np.abs(gd["F"]))))
    assert max(gaps.values()) < 1e-9, gaps
    _close(F, gd["F"], 1e-9)
    _close(G, gd["G"], 1e-6)


def test_large_long_trajectories_2048x32768(large, acc):
    """Config 2, longer horizon: 120 iterations of ABPG(gamma=2, theta_eq=True) and 60 of BPG with line
    search against traces of the real reference (oracle/gen_golden.py --only-large-long, about 1.5 h of
    CPU).  These are the solvers whose decisions are reproducible in the reference itself; the iterates
    must agree to l_inf < 1e-9 at iteration 60 and at the end."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", "large_long.npz")):
        pytest.skip("tests/golden/large_long.npz not generated")
    f, h, L, x0, _ = large
    gd = golden("large_long")
    iters, half = int(gd["iters"]), int(gd["half"])
    xh, Fh, Gh, Th = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=half, theta_eq=True, verbose=False)
    assert np.max(np.abs(xh - gd["abpg_xh"])) < 1e-9
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=iters, theta_eq=True, verbose=False)
    assert np.max(np.abs(x - gd["abpg_x"])) < 1e-9
    _close(F, gd["abpg_F"], 1e-9)
    _close(G[:half], gd["abpg_G"][:half], 1e-6)
    xb, Fb, Lb, Tb = acc.BPG(f, h, L, x0, maxitrs=half, linesearch=True, verbose=False)
    assert np.max(np.abs(xb - gd["bpgls_x"])) < 1e-9
    _close(Fb, gd["bpgls_F"], 1e-9); _close(Lb, gd["bpgls_Ls"], 1e-12)


def test_large_fw_2048x32768(large, acc):
    f, h, L, x0, _ = large
    gd = golden("large_fw")
    x, F, SP, SN, T = acc.D_opt_FW(f, x0, 1e-8, 40, verbose=False)
    assert np.max(np.abs(x - gd["fw_x"])) < 1e-9
    _close(F, gd["fw_F"], 1e-9); _close(SP, gd["fw_SP"], 1e-9)
    x, F, SP, SN, T = acc.D_opt_FW_away(f, x0, 1e-8, 40, verbose=False)
    assert np.max(np.abs(x - gd["away_x"])) < 1e-9
    _close(F, gd["away_F"], 1e-8); _close(SP, gd["away_SP"], 1e-9)


def test_factor_in_small_launches_is_the_same_arithmetic(acc):
    """accbpg_dopt_factor_in_small_launches (what the side handle of the overlapped value evaluation uses): every mode
    returns the value and gradient of the default bit for bit; mode 2 switches by size; a bad mode is refused."""
    from accbpg_and_fw_amd import _lib
    L = _lib.load()
    for m, n in [(1536, 4096), (512, 2048)]:
        V = gaussian_design(m, n, 21)
        rng = np.random.RandomState(m)
        x = rng.rand(n) + 0.01
        x /= x.sum()
        f = acc.DOptimalObj(V)
        base_f, base_g = f.func_grad(x, 2)
        for mode in (1, 2, 0):
            assert L.accbpg_dopt_factor_in_small_launches(f._h, mode) == 0
            fv, g = f.func_grad(x, 2)
            assert fv == base_f
            np.testing.assert_array_equal(g, base_g)
            assert f(x) == base_f
        assert L.accbpg_dopt_factor_in_small_launches(f._h, 3) == 4      # ACCBPG_ERR_ARG
        assert L.accbpg_dopt_factor_in_small_launches(None, 1) == 4


@pytest.mark.parametrize("fixture", ["large_fw_long", "large_fw_5000"])
def test_large_fw_1000_iterations_2048x32768(large, acc, fixture):
    """BASELINE config 3 at full length: D_opt_FW and D_opt_FW_away at (2048,32768) for 1000 iterations -- and, second
    fixture, for 5000 -- against the real reference (oracle/gen_golden.py --only-large-fw-long [--iters 5000 --name
    large_fw_5000]; accbpg/D_opt_alg.py:9-88, 91-187).  The traces hold the objective and the gaps of every iteration,
    so every vertex choice and step length along the way is pinned; D_opt_FW_away runs in its default form (F[k] anchored
    every 16th iteration, section 3.6 of DESIGN.md).
    Measured over 1000 iterations: l_inf(x) 1.7e-18 / 1.8e-18, objective traces to 3e-15 / 1e-14, gap traces to 6e-14 / 5e-14."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", fixture + ".npz")):
        pytest.skip("tests/golden/%s.npz not generated" % fixture)
    f, h, L, x0, _ = large
    gd = golden(fixture)
    iters = int(gd["iters"])
    x, F, SP, SN, T = acc.D_opt_FW(f, x0, 1e-8, iters, verbose=False)
    print("FW: l_inf %.2e, F %.2e, SP %.2e" % (np.max(np.abs(x - gd["fw_x"])), np.max(np.abs(F - gd["fw_F"]) / (1 + np.abs(gd["fw_F"]))),
                                              np.max(np.abs(SP - gd["fw_SP"]) / (1e-30 + np.abs(gd["fw_SP"])))))
    assert len(F) == len(gd["fw_F"])
    assert np.max(np.abs(x - gd["fw_x"])) < 1e-9
    _close(F, gd["fw_F"], 1e-9); _close(SP, gd["fw_SP"], 1e-7); _close(SN, gd["fw_SN"], 1e-7)
    x, F, SP, SN, T = acc.D_opt_FW_away(f, x0, 1e-8, iters, verbose=False)
    print("away: l_inf %.2e, F %.2e, SP %.2e" % (np.max(np.abs(x - gd["away_x"])), np.max(np.abs(F - gd["away_F"]) / (1 + np.abs(gd["away_F"]))),
                                                np.max(np.abs(SP - gd["away_SP"]) / (1e-30 + np.abs(gd["away_SP"])))))
    assert len(F) == len(gd["away_F"])
    assert np.max(np.abs(x - gd["away_x"])) < 1e-9
    _close(F, gd["away_F"], 1e-8); _close(SP, gd["away_SP"], 1e-7); _close(SN, gd["away_SN"], 1e-7)


@pytest.mark.parametrize("fixture", ["large_bpg_long", "large_bpg_1000"])
def test_large_bpg_ls_300_iterations_2048x32768(large, acc, fixture):
    """BPG with line search at (2048,32768) for 300 iterations -- and, second fixture, for the north star's 1000 -- against
    the real reference (oracle/gen_golden.py --only-large-bpg-long [--iters 1000 --name large_bpg_1000];
    accbpg/algorithms.py:11-72): the same L_k sequence (every accept/reject decision of the backtracking search), F[k] to
    1e-9, the final iterate to l_inf < 1e-9.  Measured over 300 iterations: l_inf 2.1e-16, F to 4.5e-13."""
    import os
    if not os.path.exists(os.path.join(os.path.dirname(__file__), "golden", fixture + ".npz")):
        pytest.skip("tests/golden/%s.npz not generated" % fixture)
    f, h, L, x0, _ = large
    gd = golden(fixture)
    iters = int(gd["iters"])
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=iters, linesearch=True, verbose=False)
    print("BPG-LS: l_inf %.2e, F %.2e" % (np.max(np.abs(x - gd["x"])), np.max(np.abs(F - gd["F"]) / (1 + np.abs(gd["F"])))))
    assert len(F) == iters
    _close(Ls, gd["Ls"], 1e-12)
    _close(F, gd["F"], 1e-9)
    assert np.max(np.abs(x - gd["x"])) < 1e-9


# ------------------------------------------------------------------ one-launch Cholesky (tile owners)
@pytest.mark.parametrize("m", [64, 100, 128, 512, 520, 1000, 1024, 1984, 2048])
def test_tile_cholesky_matches_step_kernels(acc, O, m):
    """The one-launch Cholesky (a workgroup per 64x64 tile, hand-offs inside the launch) against the launch-per-
    block-column kernels on the same matrices: the same arithmetic in the same order, so value and gradient --
    which see the factor, the log-determinant and the inverse of the factor -- are BIT-identical; and both
    against the oracle.  Ragged last blocks, one block, the largest size the scheme covers."""
    from accbpg_and_fw_amd import _lib
    n = m + 200 + (m % 7)
    V = gaussian_design(m, n, 40 + m % 13)
    rng = np.random.RandomState(m)
    f_tiles = acc.DOptimalObj(V)
    f_steps = acc.DOptimalObj(V)
    _lib.load().accbpg_debug_chol_variant(f_steps._h, 64)        # bit 6: launch per block column
    fo = O.DOptOracle(V)
    for trial in range(3):
        x = rng.rand(n) + 0.01
        x /= x.sum()
        a, ga = f_tiles.func_grad(x, 2)
        b, gb = f_steps.func_grad(x, 2)
        assert a == b
        np.testing.assert_array_equal(ga, gb)
        assert f_tiles(x) == a
        fr, gr = fo.func_grad(x, 2)
        assert abs(a - fr) < 1e-11 * max(1.0, abs(fr))
        np.testing.assert_allclose(ga, gr, rtol=1e-10)
    # not positive definite / negative entries: same error behaviour through the new path
    xz = np.zeros(n); xz[: m // 2] = 1.0 / (m // 2)
    with pytest.raises(ValueError):
        f_tiles(xz)
    xn = x.copy(); xn[3] = -1e-3
    with pytest.raises(AssertionError):
        f_tiles(xn)
    assert f_tiles(x) == a                                       # and the handle is fine afterwards


@pytest.mark.parametrize("shape", [(768, 2048), (1024, 4096), (2048, 8192), (4096, 8192)])
def test_gram_schedules_are_bit_identical(acc, shape):
    """The production Gram kernel deals its staging instructions out between MFMA pairs (placement B); the development
    switch still selects placement A and round 2's block schedule.  Same MFMAs in the same order: value and gradient are
    the same to the bit under all three (aligned stream-K ranges with dual tiles; whole tiles per workgroup at m = 4096)."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n = shape
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    f = acc.DOptimalObj(V)
    base = f.func_grad(x, 2)
    try:
        for variant in (1, 3, 2):
            lib.accbpg_debug_chol_variant(f._h, variant << 30)
            fv, g = f.func_grad(x, 2)
            assert fv == base[0], variant
            assert torch.equal(g, base[1]), variant
    finally:
        lib.accbpg_debug_chol_variant(f._h, 0)
    assert f.func_grad(x, 2)[0] == base[0]


def test_tile_cholesky_gives_up_and_redoes(acc):
    """A wait inside the one-launch Cholesky that is never satisfied (here: a test hook keeps block column 0
    unpublished) ends the launch by its bounded spin instead of hanging it; the evaluation is redone with the
    launch-per-block-column kernels and the handle stays on them."""
    import time
    from accbpg_and_fw_amd import _lib
    f, h, L, x0 = acc.D_opt_design(512, 2048, randseed=3)
    want = f.func_grad(x0, 2)
    g = acc.DOptimalObj(f.H)
    _lib.load().accbpg_debug_chol_variant(g._h, 128)             # bit 7: stall + 2 ms spin limit
    t0 = time.time()
    got = g.func_grad(x0, 2)
    assert time.time() - t0 < 5.0
    assert got[0] == want[0]
    np.testing.assert_array_equal(got[1], want[1])
    assert g(x0) == want[0]
    # the Frank-Wolfe refactorisation path (reads H in place) redoes the same way
    g2 = acc.DOptimalObj(f.H)
    _lib.load().accbpg_debug_chol_variant(g2._h, 128)
    xa, Fa, SPa, SNa, Ta = acc.D_opt_FW_away(g2, x0, 1e-8, 5, verbose=False)
    xb, Fb, SPb, SNb, Tb = acc.D_opt_FW_away(f, x0, 1e-8, 5, verbose=False)
    np.testing.assert_array_equal(xa, xb)
    np.testing.assert_array_equal(Fa, Fb)
    # ... and so do the side factorisations of F[k] = log det(H_k) (a ring of auxiliary handles, here one per iteration)
    g3 = acc.DOptimalObj(f.H)
    _lib.load().accbpg_debug_chol_variant(g3._h, 128)
    xc, Fc, SPc, SNc, Tc = acc.D_opt_FW_away(g3, x0, 1e-8, 7, verbose=False, logdet_refresh=1, logdet_ring=3)
    xd, Fd, SPd, SNd, Td = acc.D_opt_FW_away(f, x0, 1e-8, 7, verbose=False, logdet_refresh=1, logdet_ring=1)
    np.testing.assert_array_equal(xc, xd)
    np.testing.assert_array_equal(Fc, Fd)


# ------------------------------------------------------------------ sharding (one device, logical shards)
@pytest.mark.parametrize("shape,parts", [((96, 1000), 3), ((1024, 4096), 8), ((300, 1111), 4), ((2048, 8192), 4),
                                         ((4096, 16384), 2)])
def test_logical_shards_match_single_device(acc, shape, parts):
    """Design-point sharding with the all-reduce replaced by an in-process sum:
    same f and g as the unsharded objective, and a solver runs on it unchanged."""
    from accbpg_and_fw_amd.sharded import LogicalShards
    m, n = shape
    V = gaussian_design(m, n, 11)
    rng = np.random.RandomState(3)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    f = acc.DOptimalObj(V)
    fs = LogicalShards(V, parts)
    f1, g1 = f.func_grad(x, 2)
    f2, g2 = fs.func_grad(x, 2)
    assert abs(f1 - f2) < 1e-11 * max(1.0, abs(f1))
    np.testing.assert_allclose(g2, g1, rtol=1e-11)
    assert fs(x) == f2
    # accbpg/functions.py:45 on the sharded path: one negative (or NaN) entry in ONE shard raises the
    # reference's assertion, also when the summed Gram matrix is still positive definite
    for bad_value in (-1e-9, np.nan):
        xb = x.copy()
        xb[n - 2] = bad_value
        with pytest.raises(AssertionError):
            fs(xb)
    h = acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    xa, Fa, Ga, Ta = acc.ABPG(f, h, 1.0, x0, gamma=2, maxitrs=15, verbose=False)
    xb, Fb, Gb, Tb = acc.ABPG(fs, h, 1.0, x0, gamma=2, maxitrs=15, verbose=False)
    assert np.max(np.abs(xa - xb)) < 1e-12
    np.testing.assert_allclose(Fb, Fa, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape", [(96, 1001), (1024, 4096), (2048, 8192)])
def test_library_side_collectives_at_world_one(acc, shape):
    """accbpg_dopt_shard_* (the sharded evaluation with RCCL inside the library) on a communicator of one rank, which
    is what one GPU allows: the all-reduce and all-gather are identities, so f and g are bit for bit those of the
    staged evaluation with one in-process shard (and those of the unsharded objective to rounding: the staged path
    inverts the factor's diagonal blocks in a launch of its own), the assertion on x >= 0 is the reference's, and a
    solver runs on it unchanged.  (The message layout and the assembly of unequal slices are the ones
    tests/test_sharded_cpu.py covers with two ranks.)"""
    from accbpg_and_fw_amd.sharded import LogicalShards, NativeShardedDOptimalObj, native_unique_id
    m, n = shape
    V = gaussian_design(m, n, 12)
    rng = np.random.RandomState(4)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    f = acc.DOptimalObj(V)
    fs = NativeShardedDOptimalObj(torch.from_numpy(V).cuda(), n, 1, 0, native_unique_id())
    f1, g1 = f.func_grad(x, 2)
    f2, g2 = fs.func_grad(x, 2)
    f3, g3 = LogicalShards(V, 1).func_grad(x, 2)
    assert f2 == f3 and f1 == f2
    np.testing.assert_array_equal(g2, g3)
    np.testing.assert_allclose(g2, g1, rtol=1e-13)
    assert fs(x) == f2
    np.testing.assert_array_equal(fs.gradient(x), g2)
    # the gather of slices of unequal length (padded staging buffer, per-rank copies), forced here
    from accbpg_and_fw_amd import _lib
    _lib.check(_lib.load().accbpg_debug_shard_pad(fs._s, 3), "accbpg_debug_shard_pad")
    f4, g4 = fs.func_grad(x, 2)
    assert f4 == f2
    np.testing.assert_array_equal(g4, g2)
    for bad_value in (-1e-9, np.nan):
        xb = x.copy()
        xb[n - 2] = bad_value
        with pytest.raises(AssertionError):
            fs(xb)
    with pytest.raises(ValueError):
        fs(np.zeros(n))                                          # Gram matrix zero: not positive definite
    h = acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    xa, Fa, Ga, Ta = acc.ABPG(f, h, 1.0, x0, gamma=2, maxitrs=10, verbose=False)
    xb, Fb, Gb, Tb = acc.ABPG(fs, h, 1.0, x0, gamma=2, maxitrs=10, verbose=False)
    assert np.max(np.abs(xa - xb)) < 1e-12
    np.testing.assert_allclose(Fb, Fa, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("shape,K,fused", [((512, 8192), 8, True), ((256, 1024), 5, True), ((96, 640), 4, False),
                                           ((512, 1024), 20, True), ((256, 512), 1, True)])
def test_lockstep_batch_matches_sequential(acc, O, shape, K, fused):
    """BASELINE config 4 on the chip: K instances of one shape advance in lock-step, one launch per kernel family
    for all of them (accbpg_dopt_batch_*).  Every instance's run is BIT-identical to ABPG on that instance alone
    (same handle, same kernels), equal to rounding to the ordinary single-instance objective, and -- per call --
    equal to the oracle.  (96,640) is outside the fused path and is evaluated instance by instance behind the
    same interface."""
    from accbpg_and_fw_amd.batched import ABPG_batch, DOptimalBatch
    m, n = shape
    Vs = [gaussian_design(m, n, 100 + i) for i in range(K)]
    batch = DOptimalBatch(Vs)
    assert batch.fused == fused
    h = acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    iters = 25
    for kwargs in [dict(theta_eq=False), dict(theta_eq=True, restart=True)]:
        outs = ABPG_batch(batch, h, 1.0, x0, 2.0, iters, **kwargs)
        assert len(outs) == K
        for i in range(K):
            xs, Fs, Gs, Ts = acc.ABPG(batch.instance(i), h, 1.0, x0, gamma=2.0, maxitrs=iters, verbose=False, **kwargs)
            np.testing.assert_array_equal(outs[i][0], xs)
            np.testing.assert_array_equal(outs[i][1], Fs)
            np.testing.assert_array_equal(outs[i][2], Gs)
        i = K - 1
        xr, Fr, Gr, Tr = acc.ABPG(acc.DOptimalObj(Vs[i]), h, 1.0, x0, gamma=2.0, maxitrs=iters, verbose=False, **kwargs)
        assert np.max(np.abs(outs[i][0] - xr)) < 1e-11
        np.testing.assert_allclose(outs[i][1], Fr, rtol=1e-11)
    # per call against the oracle, with only some instances active
    rng = np.random.RandomState(5)
    X = rng.rand(K, n) + 0.01
    X /= X.sum(1, keepdims=True)
    active = [i % 2 == 0 for i in range(K)]
    f, G = batch.func_grad(torch.from_numpy(X).cuda(), 2, active)
    for i in range(K):
        if active[i]:
            fr, gr = O.DOptOracle(Vs[i]).func_grad(X[i], 2)
            assert abs(f[i] - fr) < 1e-11 * max(1.0, abs(fr))
            np.testing.assert_allclose(G[i].cpu().numpy(), gr, rtol=1e-10)
        else:
            assert np.isnan(f[i])
    # one bad instance raises what the sequential objective raises
    bad = K - 1
    Xb = X.copy()
    Xb[bad, 7] = -1e-3
    with pytest.raises(AssertionError):
        batch.func_grad(torch.from_numpy(Xb).cuda(), 0)
    if K > 1:
        batch.func_grad(torch.from_numpy(Xb).cuda(), 0, [i != bad for i in range(K)])   # ... unless it sits out


@pytest.mark.parametrize("shape,K,opts", [
    ((256, 1024), 5, dict(G0=0.1)),
    ((256, 1024), 3, dict(G0=0.1, ls_inc=1.5, ls_dec=1.1, theta_eq=False, restart=True)),
    ((256, 2048), 4, dict(G0=0.05, checkdiv=True, restart=True, restart_rule='f')),
    ((512, 8192), 4, dict(G0=0.1))])
def test_lockstep_abpg_gain_matches_sequential(acc, shape, K, opts):
    """ABPG_gain over a batch: one pass = one trial of every instance that is still searching; the line search
    (gain, theta, retry count) is per instance on the host and only the instances whose test failed take part in
    the next pass.  Every instance's run -- iterates, F, the gain sequence with its retries, Gdiv, Gavg -- is
    bit-identical to ABPG_gain on that instance alone, and the instances do take different numbers of retries."""
    from accbpg_and_fw_amd.batched import ABPG_gain_batch, DOptimalBatch
    m, n = shape
    Vs = [gaussian_design(m, n, 300 + 7 * i) for i in range(K)]
    batch = DOptimalBatch(Vs)
    assert batch.fused
    h = acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    iters = 45
    outs = ABPG_gain_batch(batch, h, 1.0, x0, 2, iters, **opts)
    patterns = set()
    for i in range(K):
        ref = acc.ABPG_gain(batch.instance(i), h, 1.0, x0, gamma=2, maxitrs=iters, verbose=False, **opts)
        for got, want in zip(outs[i][:-1], ref[:-1]):
            np.testing.assert_array_equal(got, want)
        gain = ref[2]
        patterns.add(tuple(np.round(np.log(gain[1:] / gain[:-1]) / np.log(opts.get("ls_inc", 1.2)), 2)))
    assert len(patterns) > 1 or K == 1                          # the instances did not all search alike


@pytest.mark.parametrize("shape,K,opts", [
    ((256, 1024), 5, dict()),
    ((256, 1024), 3, dict(linesearch=False)),
    ((256, 2048), 4, dict(ls_ratio=1.5)),
    ((512, 8192), 4, dict())])
def test_lockstep_bpg_matches_sequential(acc, O, shape, K, opts):
    """BPG over a batch (accbpg/algorithms.py:11-72 per instance): one (f, grad) launch for all running instances,
    then one prox + one trial value per pass of the backtracking search for the instances still searching.  Every
    instance's run -- iterates, F and the L_k sequence with its retries -- is bit-identical to BPG on that instance
    alone, the instances do search differently, and one instance's F agrees with the oracle-backed solver."""
    from accbpg_and_fw_amd.batched import BPG_batch, DOptimalBatch
    m, n = shape
    Vs = [gaussian_design(m, n, 500 + 11 * i) for i in range(K)]
    batch = DOptimalBatch(Vs)
    assert batch.fused
    h = acc.BurgEntropySimplex()
    x0 = np.ones(n) / n
    iters = 40
    outs = BPG_batch(batch, h, 1.0, x0, iters, **opts)
    assert len(outs) == K
    patterns = set()
    for i in range(K):
        ref = acc.BPG(batch.instance(i), h, 1.0, x0, maxitrs=iters, verbose=False, **opts)
        for got, want in zip(outs[i][:-1], ref[:-1]):
            np.testing.assert_array_equal(got, want)
        patterns.add(tuple(ref[2]))
    if opts.get("linesearch", True):
        assert len(patterns) > 1                                 # the instances did not all search alike
    # one instance against the CPU restatement of the solver (same L_k decisions, F to rounding)
    xo, Fo, Lo, To = O.BPG(O.DOptOracle(Vs[0]), O.BurgSimplexOracle(), 1.0, x0, iters, **opts)
    np.testing.assert_array_equal(outs[0][2], Lo)
    np.testing.assert_allclose(outs[0][1], Fo, rtol=1e-10)
    assert np.max(np.abs(outs[0][0] - xo)) < 1e-12


def test_batch_size_limit_is_a_clean_error(acc):
    """A batch holds at most ACCBPG_BATCH_MAX = 64 instances (the active set travels as a fixed-size kernel argument):
    one more is refused at creation with ACCBPG_ERR_ARG -> ValueError, 64 are accepted and evaluate."""
    from accbpg_and_fw_amd.batched import DOptimalBatch
    gen = torch.Generator(device="cuda").manual_seed(1)
    Vs = [torch.randn(64, 256, dtype=torch.float64, device="cuda", generator=gen) for _ in range(65)]
    with pytest.raises(ValueError, match="at most"):
        DOptimalBatch(Vs)
    b = DOptimalBatch(Vs[:64])
    x = torch.full((64, 256), 1.0 / 256, dtype=torch.float64, device="cuda")
    fv, g = b.func_grad(x, flag=2)
    assert np.all(np.isfinite(fv))
    one = acc.DOptimalObj(Vs[63]).func_grad(x[63], 2)
    assert fv[63] == pytest.approx(one[0], rel=1e-12)


def test_batched_instances_match_sequential(acc):
    """Config-4 style batch: independent instances solved concurrently from host threads on
    separate streams give exactly the results of solving them one after the other."""
    from accbpg_and_fw_amd.batched import solve_batch
    probs = [acc.D_opt_design(96, 640, randseed=50 + j) for j in range(6)]
    seq = [acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=40, verbose=False) for f, h, L, x0 in probs]
    par = solve_batch(probs, acc.ABPG_gain, threads=6, gamma=2, maxitrs=40, verbose=False)
    for a, b in zip(seq, par):
        np.testing.assert_array_equal(a[0], b[0])          # same kernels, same order per instance -> bitwise
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])


def test_batched_fresh_instances_match_sequential(acc):
    """The same with objects the threads are the first to touch: the sequential leg runs on problems of its own from
    the same seeds, so no handle of the parallel leg has been evaluated before -- its first evaluation, its first trial
    (the lazily allocated status block) and its side handle all happen on the threads' non-blocking streams."""
    from accbpg_and_fw_amd.batched import solve_batch
    seq_probs = [acc.D_opt_design(96, 640, randseed=50 + j) for j in range(6)]
    seq = [acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=40, verbose=False) for f, h, L, x0 in seq_probs]
    probs = [acc.D_opt_design(96, 640, randseed=50 + j) for j in range(6)]      # never evaluated
    par = solve_batch(probs, acc.ABPG_gain, threads=6, gamma=2, maxitrs=40, verbose=False)
    for a, b in zip(seq, par):
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])
        np.testing.assert_array_equal(a[2], b[2])


# ------------------------------------------------------------------ SURVEY 8(f) rows 1-3
import os as _os
_DATA = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden", "data")


def test_libsvm_instances_gpu(acc):
    """D_opt_libsvm on the four vendored files: F(x0) as the reference computes it."""
    gd = golden("next_rows")
    for name in ["housing", "bodyfat", "mpg", "abalone"]:
        f, h, L, x0 = acc.D_opt_libsvm(_os.path.join(_DATA, name + ".txt"))
        assert f.H.shape == tuple(gd["libsvm_%s_shape" % name])
        assert f(x0) == pytest.approx(float(gd["libsvm_%s_f0" % name]), rel=1e-11)


def test_expo_abda_fwdiv_trajectories(acc):
    """ABPG_expo, ABDA and FW_alg_div_step + lmo_simplex with the calls of
    frank_wolfe_wtih_rs/ex_Dopt_design.py:12-21 (housing) and on D_opt_design(80,200,seed 10)."""
    gd = golden("next_rows")
    f, h, L, x0 = acc.D_opt_libsvm(_os.path.join(_DATA, "housing.txt"))
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=300, linesearch=True, ls_ratio=2, verbose=False)
    _close(F, gd["h_bpg_F"], 1e-9); _close(Ls, gd["h_bpg_Ls"], 1e-12)
    x, F, Ls, T = acc.FW_alg_div_step(f, h, L, x0, lmo=acc.lmo_simplex(), maxitrs=300, gamma=2.0, ls_ratio=2,
                                      verbose=False)
    k = _agree_prefix(Ls, gd["h_fwdiv_Ls"], 1e-12)
    assert k >= 150, k
    _close(F[:k], gd["h_fwdiv_F"][:k], 1e-9)
    x, F, Gamma, G, T = acc.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=300, theta_eq=True, Gmargin=100, verbose=False)
    k = _agree_prefix(Gamma, gd["h_expo_Gamma"], 1e-12)
    assert k >= 100, k
    _close(F[:100], gd["h_expo_F"][:100], 1e-9)
    f, h, L, x0 = acc.D_opt_design(80, 200, randseed=10)
    x, F, Gamma, G, T = acc.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=300, theta_eq=True, verbose=False)
    k = _agree_prefix(Gamma, gd["r_expo_Gamma"], 1e-12)
    assert k >= 200, k
    _close(F[:200], gd["r_expo_F"][:200], 1e-9)
    assert len(F) == len(Gamma) == len(G) == len(T)
    x, F, Gamma, G, T = acc.ABPG_expo(f, h, L, x0, gamma0=2.5, maxitrs=200, theta_eq=False, checkdiv=True,
                                      Gmargin=5, restart=True, verbose=False)
    k = _agree_prefix(Gamma, gd["r_expo2_Gamma"], 1e-12)
    assert k >= 40, k
    _close(F[:40], gd["r_expo2_F"][:40], 1e-9)
    x, F, G, T = acc.ABDA(f, h, L, x0, gamma=2, maxitrs=300, theta_eq=True, verbose=False)
    _close(F, gd["r_abda_F"], 1e-9)
    assert np.max(np.abs(x - gd["r_abda_x"])) < 1e-9
    x, F, Ls, T = acc.FW_alg_div_step(f, h, L, x0, lmo=acc.lmo_simplex(), maxitrs=300, gamma=2.0, ls_ratio=2,
                                      verbose=False)
    k = _agree_prefix(Ls, gd["r_fwdiv_Ls"], 1e-12)
    assert k >= 150, k
    _close(F[:k], gd["r_fwdiv_F"][:k], 1e-9)
    with pytest.raises(ValueError):
        acc.FW_alg_div_step(f, h, -1.0, x0, 5, 2.0, acc.lmo_simplex(), verbose=False)


def test_lmo_simplex_and_argminmax(acc):
    from accbpg_and_fw_amd.functions import vec_argminmax, vec_div_scalar
    rng = np.random.RandomState(8)
    for n in [5, 1000, 70001]:
        g = rng.randn(n)
        g[rng.randint(n)] = g.min()                 # a tie: the first index must win
        s = acc.lmo_simplex(2.0)(g)
        ref = np.zeros(n) + 1e-15
        ref[np.where(g == g.min())[0][0]] = 2.0
        np.testing.assert_array_equal(s, ref)
        imin, imax, vmin, vmax = vec_argminmax(dev(g))
        assert imin == np.argmin(g) and imax == np.argmax(g) and vmin == g.min() and vmax == g.max()
        np.testing.assert_array_equal(vec_div_scalar(dev(g), 3.7).cpu().numpy(), g / 3.7)


def test_kyinit_gpu(acc):
    """Kumar-Yildirim start: identical support and weights to the reference for the same RNG state,
    and FW-away started from it follows the reference's trajectory."""
    gd = golden("next_rows")
    f, h, L, x0 = acc.D_opt_design(30, 1000, randseed=4)
    np.random.seed(99)
    xky = acc.D_opt_KYinit(f.H)
    np.testing.assert_array_equal(xky, gd["ky_x"])
    np.random.seed(99)
    np.testing.assert_array_equal(acc.D_opt_KYinit(f), gd["ky_x"])        # also accepts the objective
    np.testing.assert_array_equal(acc.D_opt_KYinit(np.zeros((30, 60))), np.ones(60) / 60)
    xs, F, SP, SN, T = acc.D_opt_FW_away(f.H, xky, 1e-8, 2000, verbose=False)
    k = min(len(F), len(gd["ky_away_F"]))
    assert abs(len(F) - len(gd["ky_away_F"])) <= 2
    _close(F[:k], gd["ky_away_F"][:k], 1e-8)
    assert np.max(np.abs(xs - gd["ky_away_x"])) < 1e-8


# ------------------------------------------------------------------ Gram-matrix reuse through linearity
@pytest.mark.parametrize("solver", ["abpg", "abpg_gain", "abpg_restart"])
def test_linear_gram_reuse_matches_direct(acc, solver):
    """Opt-in extension: V diag(x) V^T is linear in x, so the accelerated solvers can combine resident
    Gram matrices instead of re-forming them.  Same trajectory as direct evaluation to rounding, with
    one O(m^2 n) product per pass instead of two or three."""
    gd = golden("traces_80x200")
    f, h, L, x0 = acc.D_opt_design(80, 200, randseed=10)
    if solver == "abpg":
        run = lambda ff: acc.ABPG(ff, h, L, x0, gamma=2.0, maxitrs=400, theta_eq=True, verbose=False)
        ref_x, ref_F = None, gd["abpg_F"][:400]
    elif solver == "abpg_restart":
        run = lambda ff: acc.ABPG(ff, h, L, x0, gamma=2.0, maxitrs=400, theta_eq=True, restart=True, verbose=False)
        ref_x, ref_F = None, gd["abpgrs_F"][:400]
    else:
        run = lambda ff: acc.ABPG_gain(ff, h, L, x0, gamma=2, maxitrs=400, G0=0.1, theta_eq=True, verbose=False)
        ref_x, ref_F = None, gd["gain_F"][:400]
    base = run(f)
    f2 = acc.DOptimalObj(f.H).linear_gram(True, refresh=25)
    lin = run(f2)
    assert np.max(np.abs(lin[0] - base[0])) < 1e-11
    np.testing.assert_allclose(lin[1], base[1], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(lin[1], ref_F, rtol=1e-9, atol=1e-9)          # and the reference's trace
    evals = f2.calls["value"] + f2.calls["grad"]
    assert f2.gram_launches + f2.gram_combos <= evals + 450
    assert f2.gram_launches < 0.62 * evals, (f2.gram_launches, f2.gram_combos, evals)
    # plain evaluations still work on an object with reuse enabled
    fx, g = f2.func_grad(x0, 2)
    fb, gb = f.func_grad(x0, 2)
    assert fx == fb
    np.testing.assert_array_equal(g, gb)


def test_trajectories_512x8192(acc):
    """1000-iteration l_inf parity at the BASELINE config-4 instance size D_opt_design(512,8192)
    (traces from the real reference, /tmp generation script of oracle/gen_golden.py style)."""
    gd = golden("traces_512x8192")
    f, h, L, x0 = acc.D_opt_design(512, 8192, randseed=10)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=1000, linesearch=True, verbose=False)
    assert np.max(np.abs(x - gd["bpgls_x"])) < 1e-9
    _close(F, gd["bpgls_F"], 1e-9); _close(Ls, gd["bpgls_Ls"], 1e-12)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=1000, theta_eq=True, verbose=False)
    assert np.max(np.abs(x - gd["abpg_x"])) < 1e-9
    _close(F, gd["abpg_F"], 1e-9)
    x, F, Gain, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=300, verbose=False)
    k = _agree_prefix(Gain, gd["gain_Gain"], 1e-12)
    assert k >= 25, k
    _close(F[:25], gd["gain_F"][:25], 1e-9)


def test_config5_shard_shape_properties(acc):
    """One rank's share of BASELINE config 5 -- m = 8192, 32768 local design points (2 GiB of V, 128 block
    columns in the Cholesky, seven merge levels, a Gram tile list of 1040 entries walked in ranges longer
    than a tile): size-independent identities, no CPU pass.  sum_i x_i (-g_i) = m exactly, and
    f(c x) = f(x) - m log c."""
    m, n = 8192, 32768
    gen = torch.Generator(device="cuda").manual_seed(8)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    f = acc.DOptimalObj(V)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.1
    x /= x.sum()
    fx, g = f.func_grad(x, 2)
    assert np.isfinite(fx)
    assert float(-(x * g).sum()) == pytest.approx(m, rel=1e-10)
    assert f(2.5 * x) == pytest.approx(fx - m * np.log(2.5), rel=1e-12)
    g2 = f.gradient(2.5 * x)
    assert float((g2 * 2.5 - g).abs().max() / g.abs().max()) < 1e-10      # gradient is (-1)-homogeneous
    del V, f


def test_m8192_matches_reference_golden(acc):
    """BASELINE config 5's m against the REAL reference: D_opt_design(8192,16400,seed 10) -- 128 block columns in the
    two-level Cholesky, seven levels of inverse merges, a ragged last column tile in the gradient product -- func_grad at
    x0 and at a random point, and three ABPG iterations (oracle/gen_golden.py --only-m8192; accbpg/functions.py:43-59,
    accbpg/algorithms.py:94-180), on the plain objective AND through eight logical shards (unequal slices: 16400 = 8 *
    2050) with the all-reduce replaced by an in-process sum of the packed triangles."""
    from accbpg_and_fw_amd.sharded import LogicalShards
    gd = golden("percall_8192x16400")
    m, n = int(gd["m"]), int(gd["n"])
    V = torch.from_numpy(gaussian_design(m, n, int(gd["seed"]))).cuda()
    x0 = np.ones(n) / n
    f = acc.DOptimalObj(V)
    fs = LogicalShards(V, 8)
    for obj, name in ((f, "plain"), (fs, "8 logical shards")):
        f0, g0 = obj.func_grad(x0, 2)
        fx, g = obj.func_grad(gd["x"], 2)
        print("%s: rel gap f0 %.2e f %.2e, g0 %.2e g %.2e" % (
            name, abs(f0 - float(gd["f0"])) / abs(float(gd["f0"])), abs(fx - float(gd["f"])) / abs(float(gd["f"])),
            np.max(np.abs(g0 - gd["g0"]) / np.abs(gd["g0"])), np.max(np.abs(g - gd["g"]) / np.abs(gd["g"]))))
        assert abs(f0 - float(gd["f0"])) < 1e-11 * abs(float(gd["f0"]))
        assert abs(fx - float(gd["f"])) < 1e-11 * abs(float(gd["f"]))
        np.testing.assert_allclose(g0, gd["g0"], rtol=1e-11)
        np.testing.assert_allclose(g, gd["g"], rtol=1e-11)
        assert obj(gd["x"]) == pytest.approx(float(gd["f"]), rel=1e-11)
    h = acc.BurgEntropySimplex()
    iters = int(gd["iters"])
    for obj in (f, fs):
        x, F, G, T = acc.ABPG(obj, h, 1.0, x0, gamma=2, maxitrs=iters, theta_eq=True, verbose=False)
        assert np.max(np.abs(x - gd["abpg_x"])) < 1e-12
        _close(F, gd["abpg_F"], 1e-11)
    del f, fs, V


def test_config5_full_size_8192x262144(acc, O):
    """BASELINE config 5 at ITS size on one GPU: D_opt_design-shaped (8192,262144), V = 16 GiB resident (standard normal,
    generated on the device).  The sharded evaluation -- eight logical shards, each rank's packed Gram triangle and x >= 0
    count summed in process where RCCL would all-reduce them, replicated two-level Cholesky, per-shard gradient slices --
    against the unsharded objective on the same V: f to 1e-11, g to rtol 1e-11; the trace identity sum_i x_i (-g_i) = m and
    f(c x) = f(x) - m log c; the reference's x >= 0 assertion from one bad entry in one shard; the multi-workgroup Burg prox
    at n = 262144 against the oracle's scalar loop; three ABPG iterations sharded vs unsharded to l_inf < 1e-12; and
    accbpg_dopt_shard_* (RCCL inside the library) on a communicator of one rank at this size, bit for bit the staged
    evaluation."""
    from accbpg_and_fw_amd.sharded import LogicalShards, NativeShardedDOptimalObj, native_unique_id
    m, n, parts = 8192, 262144, 8
    gen = torch.Generator(device="cuda").manual_seed(5)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.1
    x /= x.sum()
    f = acc.DOptimalObj(V)
    f1, g1 = f.func_grad(x, 2)
    assert np.isfinite(f1)
    assert float(-(x * g1).sum()) == pytest.approx(m, rel=1e-10)
    assert f(2.5 * x) == pytest.approx(f1 - m * np.log(2.5), rel=1e-12)
    fs = LogicalShards(V, parts)
    f2, g2 = fs.func_grad(x, 2)
    print("sharded vs unsharded at (8192,262144): rel gap f %.2e, g %.2e"
          % (abs(f1 - f2) / abs(f1), float(((g2 - g1).abs() / g1.abs()).max())))
    assert abs(f1 - f2) < 1e-11 * abs(f1)
    assert float(((g2 - g1).abs() / g1.abs()).max()) < 1e-11
    assert fs(x) == f2
    assert float(-(x * g2).sum()) == pytest.approx(m, rel=1e-10)
    for bad_value in (-1e-9, float("nan")):
        xb = x.clone()
        xb[n - 2] = bad_value                                    # one entry, in the last shard only
        with pytest.raises(AssertionError):
            fs(xb)
        with pytest.raises(AssertionError):
            f(xb)
    # the prox of the solver step at this n (several workgroups; accbpg/functions.py:336-356)
    h = acc.BurgEntropySimplex()
    z = h.div_prox_map(x, g1, 1.0)
    zo = O.BurgSimplexOracle().div_prox_map(x.cpu().numpy(), g1.cpu().numpy(), 1.0)
    np.testing.assert_allclose(z.cpu().numpy(), zo, rtol=1e-11)
    assert abs(float(z.sum()) - 1) <= 1.001e-8 and float(z.min()) > 0
    x0 = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    xa, Fa, Ga, Ta = acc.ABPG(f, h, 1.0, x0, gamma=2, maxitrs=3, verbose=False)
    xb, Fb, Gb, Tb = acc.ABPG(fs, h, 1.0, x0, gamma=2, maxitrs=3, verbose=False)
    assert float((xa - xb).abs().max()) < 1e-12
    np.testing.assert_allclose(Fb, Fa, rtol=1e-12)
    del fs
    torch.cuda.empty_cache()
    fn = NativeShardedDOptimalObj(V, n, 1, 0, native_unique_id())
    f3, g3 = fn.func_grad(x, 2)
    f4, g4 = LogicalShards(V, 1).func_grad(x, 2)
    assert f3 == f4
    assert torch.equal(g3, g4)
    assert abs(f3 - f1) < 1e-11 * abs(f1)
    assert float(((g3 - g1).abs() / g1.abs()).max()) < 1e-11
    del fn, f, V
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(300, 3000), (1024, 4096), (4160, 8320)])
def test_runs_are_bitwise_reproducible(acc, shape):
    """Fixed reduction trees, a deterministic stream-K fix-up order and no unordered atomics (the
    log-determinant takes one device-scope add per launch, in launch order): the same solver run gives the
    same bits every time (small-tile path, big-tile path with dual tiles, two-level Cholesky)."""
    f, h, L, x0 = acc.D_opt_design(shape[0], shape[1], randseed=21)
    its = 40 if shape[0] < 2000 else 12
    ref = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=its, verbose=False)
    for _ in range(3):
        again = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=its, verbose=False)
        for p, q in zip(ref[:-1], again[:-1]):
            np.testing.assert_array_equal(p, q)


@pytest.mark.parametrize("shape", [(300, 3000), (512, 8192), (1024, 4096), (1536, 4096), (2048, 8192)])
def test_overlapped_value_evaluation_is_identical(acc, shape):
    """The default: F[k] = f(x) on a side stream beside func_grad(y).  Same kernels on the same data, so
    the whole run is bitwise identical to the one with both evaluations on the solver's stream.  The last two
    shapes lie above the size (m > 1408) from which the side handle factors in small launches."""
    f, h, L, x0 = acc.D_opt_design(shape[0], shape[1], randseed=21)
    assert f._overlap                                           # on unless switched off
    f.overlap_values(False)
    a = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=60, verbose=False)
    b = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=60, theta_eq=True, restart=True, verbose=False)
    f.overlap_values(True)
    a2 = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=60, verbose=False)
    b2 = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=60, theta_eq=True, restart=True, verbose=False)
    for u, v in [(a, a2), (b, b2)]:
        for p, q in zip(u[:-1], v[:-1]):
            np.testing.assert_array_equal(p, q)
    # an error inside the overlapped evaluation surfaces at the wait
    bad = torch.from_numpy(-x0).cuda()
    with pytest.raises(AssertionError):
        f.value_wait(f.value_async(bad))


@pytest.mark.parametrize("overlap", [False, True])
def test_memoized_values_change_nothing(acc, overlap):
    """DOptimalObj.memoize_values (opt-in): F[k+1] = f(x) at the accepted line-search point (accbpg/algorithms.py:347) is
    answered from the value the accepting test computed at that very tensor (:387) instead of a second evaluation.  Every
    trace is bit-identical to the run without it, one value evaluation per iteration is saved, and a tensor that was
    modified in place or merely equal in content is evaluated afresh."""
    f, h, L, x0 = acc.D_opt_design(300, 3000, randseed=4)
    f.overlap_values(overlap)
    a = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=80, verbose=False)
    b0 = acc.BPG(f, h, L, x0, maxitrs=40, linesearch=True, verbose=False)
    v0 = f.calls["value"]
    f.memoize_values(True)
    hits0 = f.value_hits
    b = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=80, verbose=False)
    hits = f.value_hits - hits0
    b1 = acc.BPG(f, h, L, x0, maxitrs=40, linesearch=True, verbose=False)
    for p, q in list(zip(a[:-1], b[:-1])) + list(zip(b0[:-1], b1[:-1])):
        np.testing.assert_array_equal(p, q)
    assert 70 <= hits <= 80                                     # every F[k], k >= 1, of the ABPG_gain run
    xd = torch.from_numpy(x0).cuda()
    v = f(xd)
    assert f(xd) == v and f.value_hits > hits0 + hits           # the same object again: answered
    xd.mul_(1.5)                                                # modified in place: evaluated afresh
    assert f(xd) == pytest.approx(v - f.m * np.log(1.5), rel=1e-12)
    assert f(xd.clone()) == f(xd)                               # equal content, another object: evaluated (same value)
    f.memoize_values(False)


@pytest.mark.parametrize("shape,opts", [((300, 3000), dict(gamma=2)), ((512, 8192), dict(gamma=2, G0=0.1)),
                                        ((256, 4096), dict(gamma=2, ls_inc=1.5, ls_dec=1.1, theta_eq=False, restart=True)),
                                        ((128, 1024), dict(gamma=1.5, G0=0.1, restart=True, restart_rule='f'))])
def test_gradients_started_ahead_change_nothing(acc, shape, opts):
    """ABPG_gain starts the next trial's gradient evaluation beside the current value test when the previous
    iteration needed that retry (DOptimalObj.speculate, default).  Every evaluation that is used is the one the
    sequential loop makes: the whole run is bit-identical to the run without it, the oracle-call counts are the
    same, and once the search has settled into its retry pattern few started evaluations go unused."""
    f, h, L, x0 = acc.D_opt_design(shape[0], shape[1], randseed=8)
    iters = 150
    f.speculate(False)
    c0 = dict(f.calls)
    a = acc.ABPG_gain(f, h, L, x0, maxitrs=iters, verbose=False, **opts)
    calls_plain = {k: f.calls[k] - c0[k] for k in c0}
    f.speculate(True)
    c0 = dict(f.calls); unused0 = f.spec_unused
    b = acc.ABPG_gain(f, h, L, x0, maxitrs=iters, verbose=False, **opts)
    calls_ahead = {k: f.calls[k] - c0[k] for k in c0}
    for p, q in zip(a[:-1], b[:-1]):
        np.testing.assert_array_equal(p, q)
    assert calls_plain == calls_ahead
    retries = calls_plain["grad"] - len(a[1])
    assert retries > 20                                        # the runs do retry
    assert f.spec_unused - unused0 <= 0.5 * retries + 5        # and most evaluations started ahead were used


@pytest.mark.parametrize("overlap", [False, True])
@pytest.mark.parametrize("solver", ["abpg", "abpg_gain"])
def test_time_stamps_mark_when_F_was_known(acc, overlap, solver):
    """T[k] is stamped when F[k] = f(x) is known, as the reference does right after computing it
    (accbpg/algorithms.py:135-137, 347-349) -- not after the gradient evaluation that follows.  The gradient is
    delayed by 60 ms on the host: T[0] must not contain that delay, later gaps must."""
    import time
    f, h, L, x0 = acc.D_opt_design(256, 4096, randseed=5)
    f.overlap_values(overlap)
    f.func_grad(x0, 2)                                          # first-use costs out of the way
    if overlap:
        f.value_wait(f.value_async(torch.from_numpy(x0).cuda()))
    slow = f.func_grad

    def delayed(x, flag=2):
        if flag != 0:
            time.sleep(0.06)
        return slow(x, flag)

    f.func_grad = delayed
    f.gradient = lambda x: delayed(x, 1)
    try:
        t0 = time.time()
        if solver == "abpg":
            out = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=4, verbose=False)
        else:
            out = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=4, verbose=False)
        wall = time.time() - t0
    finally:
        del f.func_grad, f.gradient
    T = out[-1]
    assert 0 <= T[0] < 0.045, T                                 # the first value was known before the slow gradient
    assert np.all(np.diff(T) >= 0.055) and T[-1] <= wall        # every later stamp has one delay more behind it


# ------------------------------------------------------------------ Poisson + Burg L1/L2
_POISSON = {"l1": ("Poisson_regrL1", 200, 100, 0.0001, 0), "l2": ("Poisson_regrL2", 100, 1000, 0.001, 0.001),
            "l1r": ("Poisson_regrL1", 300, 2000, 0.001, 0.01)}


def _poisson(mod, tag):
    """The factory's instance with b and L pinned to the golden run: the factory forms b = A x + noise with
    the HOST BLAS (as the reference does), whose dot products differ by an ulp from machine to machine."""
    fac, m, n, noise, lam = _POISSON[tag]
    f, h, L, x0 = getattr(mod, fac)(m, n, noise=noise, lamda=lam, randseed=1)
    gd = golden("poisson")
    np.testing.assert_allclose(f.b, gd[tag + "_b"], rtol=1e-13)   # same legacy-RNG draw order as the factory
    assert L == pytest.approx(float(gd[tag + "_L"]), rel=1e-13)
    np.testing.assert_array_equal(x0, gd[tag + "_x0"])
    return type(f)(f.A, gd[tag + "_b"]), h, float(gd[tag + "_L"]), x0


@pytest.mark.parametrize("tag", ["l1", "l2", "l1r"])
def test_poisson_percall_matches_reference_golden(acc, tag):
    """PoissonRegression.func_grad and the closed-form Burg L1/L2 prox maps against vectors written by the
    real reference.  The matrix-vector products differ from BLAS by summation order (1e-14 relative); the
    prox maps are elementwise with NumPy's operation order, so they are bit-exact on identical inputs."""
    gd = golden("poisson")
    f, h, L, x0 = _poisson(acc, tag)
    x, y = gd[tag + "_x"], gd[tag + "_y"]
    fx, g = f.func_grad(x, 2)
    assert fx == pytest.approx(float(gd[tag + "_f"]), rel=1e-13, abs=1e-14)
    np.testing.assert_allclose(g, gd[tag + "_g"], rtol=1e-12, atol=1e-13)
    assert f(x) == fx
    np.testing.assert_array_equal(f.gradient(x), g)
    assert f(x0) == pytest.approx(float(gd[tag + "_f0"]), rel=1e-13, abs=1e-14)
    np.testing.assert_allclose(f.gradient(x0), gd[tag + "_g0"], rtol=1e-12, atol=1e-13)
    np.testing.assert_allclose(f.fitted(), f.A @ x0, rtol=1e-13)
    assert h.extra_Psi(x) == pytest.approx(float(gd[tag + "_psi"]), rel=1e-14)
    for idx in range(3):
        z = h.div_prox_map(y, gd[tag + "_g"], float(gd["%s_prox_L%d" % (tag, idx)]))
        np.testing.assert_array_equal(z, gd["%s_prox_x%d" % (tag, idx)])
    np.testing.assert_array_equal(h.prox_map(np.abs(gd[tag + "_g"]) + 0.5, 2.0), gd[tag + "_prox_raw"])
    assert h.divergence(x, y) == pytest.approx(float(gd[tag + "_div_xy"]), rel=1e-13)
    xd = dev(x)                                                    # device vectors stay on the device
    fd, gdv = f.func_grad(xd, 2)
    assert isinstance(gdv, torch.Tensor) and gdv.is_cuda and fd == fx
    np.testing.assert_array_equal(gdv.cpu().numpy(), g)


@pytest.mark.parametrize("shape", [(37, 51), (64, 5001), (5, 4096), (1000, 3), (513, 130)])
def test_poisson_shapes_against_oracle(acc, O, shape):
    """Odd sizes (scalar-load path), few long rows (workgroup-per-row path), tall thin matrices."""
    m, n = shape
    rng = np.random.RandomState(m + 3 * n)
    A = rng.rand(m, n)
    b = rng.rand(m) + 0.1
    x = rng.rand(n) / n + 1e-4
    fo, go = O.PoissonOracle(A, b).func_grad(x, 2)
    f = acc.PoissonRegression(A, b)
    fx, g = f.func_grad(x, 2)
    assert fx == pytest.approx(fo, rel=1e-13)
    np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-13 * np.abs(go).max())


def test_poisson_long_rows_branch_against_oracle(acc, O):
    """(2048, 32768), 512 MiB of A: the wave-per-row A x kernel with its occupancy-limiting LDS request
    (m >= 8 CUs' worth of rows, n >= 32768) and the A^T r pass at that shape's row split, against the oracle:
    A x, f and g."""
    m, n = 2048, 32768
    rng = np.random.RandomState(12)
    A = rng.rand(m, n)
    b = rng.rand(m) + 0.1
    x = rng.rand(n) / n + 1e-5
    fo, go = O.PoissonOracle(A, b).func_grad(x, 2)
    f = acc.PoissonRegression(A, b)
    fx, g = f.func_grad(x, 2)
    np.testing.assert_allclose(f.fitted(), A @ x, rtol=1e-12)
    assert fx == pytest.approx(fo, rel=1e-12)
    np.testing.assert_allclose(g, go, rtol=1e-12, atol=1e-13 * np.abs(go).max())
    assert f(x) == fx


def test_poisson_leading_dimension_through_c_abi(acc, O):
    """lda > n and an unaligned base pointer, straight through the C-ABI."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n, lda = 70, 301, 333
    rng = np.random.RandomState(5)
    buf = rng.rand(m * lda + 1)
    A = buf[1:].reshape(m, lda)[:, :n]
    b = rng.rand(m) + 0.2
    x = rng.rand(n) / n + 1e-4
    fo, go = O.PoissonOracle(np.ascontiguousarray(A), b).func_grad(x, 2)
    bufd, bd, xd = dev(buf), dev(b), dev(x)
    g = torch.empty(n, dtype=torch.float64, device="cuda")
    h = C.c_void_p()
    assert lib.accbpg_poisson_create(bufd.data_ptr() + 8, m, n, lda, bd.data_ptr(), None, C.byref(h)) == 0
    fv = C.c_double()
    assert lib.accbpg_poisson_func_grad(h, xd.data_ptr(), 2, C.byref(fv), g.data_ptr()) == 0
    torch.cuda.synchronize()
    assert fv.value == pytest.approx(fo, rel=1e-13)
    np.testing.assert_allclose(g.cpu().numpy(), go, rtol=1e-12)
    assert lib.accbpg_poisson_func_grad(h, xd.data_ptr(), 3, C.byref(fv), g.data_ptr()) == _lib.ERR_ARG
    assert lib.accbpg_poisson_create(bufd.data_ptr(), m, n, n - 1, bd.data_ptr(), None, C.byref(C.c_void_p())) \
        == _lib.ERR_ARG
    lib.accbpg_poisson_destroy(h)


def test_poisson_and_burg_errors(acc):
    """The reference's assertions (functions.py:90, 103, 260-261, 270, 279, 295-296, 306, 320)."""
    rng = np.random.RandomState(0)
    A, b = rng.rand(20, 30), rng.rand(20) + 0.1
    with pytest.raises(AssertionError):
        acc.PoissonRegression(A, b[:-1])
    f = acc.PoissonRegression(A, b)
    with pytest.raises(AssertionError):
        f.func_grad(np.ones(29))
    g = np.linspace(-0.5, 2.0, 30)
    y = np.full(30, 0.1)
    h1 = acc.BurgEntropyL1(0.25)
    with pytest.raises(AssertionError, match="positive solution"):
        h1.prox_map(g, 1.0)                                     # g.min() = -0.5 <= -lamda
    assert np.all(h1.prox_map(g + 0.3, 1.0) > 0)
    np.testing.assert_array_equal(h1.prox_map(g + 0.3, 2.0), 2.0 / (0.25 + (g + 0.3)))
    with pytest.raises(AssertionError):
        h1.prox_map(g + 1.0, 0.0)
    with pytest.raises(AssertionError):
        h1.div_prox_map(y * 0.0, g, 1.0)                        # y not positive
    with pytest.raises(AssertionError):
        h1.div_prox_map(y[:-1], g, 1.0)
    with pytest.raises(AssertionError):
        acc.BurgEntropyL1(-1.0)
    with pytest.raises(AssertionError):
        acc.BurgEntropyL2(-1.0)
    h0 = acc.BurgEntropy()
    with pytest.raises(AssertionError, match="positive value"):
        h0.prox_map(g, 1.0)
    np.testing.assert_array_equal(h0.prox_map(g + 1.0, 3.0), 3.0 / (g + 1.0))
    np.testing.assert_array_equal(h0.div_prox_map(y, g, 3.0), 3.0 / (g - 3.0 * (-1 / y)))
    h2 = acc.BurgEntropyL2(0.5)
    with pytest.raises(AssertionError):
        h2.prox_map(g, -1.0)
    gg, lam_L = g / 3.0, 0.5 / 3.0
    np.testing.assert_array_equal(h2.prox_map(g, 3.0), (np.sqrt(gg * gg + 4 * lam_L) - gg) / (2 * lam_L))
    assert acc.BurgEntropyL1(0).extra_Psi(y) == 0 and acc.BurgEntropyL2(0).extra_Psi(y) == 0
    assert h2.extra_Psi(y) == pytest.approx(0.25 * np.dot(y, y), rel=1e-15)
    assert h1.extra_Psi(y) == pytest.approx(0.25 * y.sum(), rel=1e-15)


def test_poisson_l1_trajectories(acc):
    """ipynb/ex_Poisson_L2.ipynb cells 1 and 3 at Poisson_regrL1(200, 100, noise=1e-4, lamda=0, randseed=1),
    2000 iterations each (measured deviations from the reference: x 1e-16, F 4e-15; ABPG_expo's exponent
    decisions part ways with the reference's at k = 468, see _check_gain_runs for why)."""
    gd = golden("poisson")
    f, h, L, x0 = _poisson(acc, "l1")
    N = 2000
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=N, linesearch=False, verbose=False)
    assert np.max(np.abs(x - gd["l1_bpg_x"])) < 1e-12
    _close(F, gd["l1_bpg_F"], 1e-12)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=N, linesearch=True, verbose=False)
    k = _agree_prefix(Ls, gd["l1_bpgls_Ls"], 1e-12)
    assert k >= 500, k
    _close(F[:k], gd["l1_bpgls_F"][:k], 1e-11)
    for gam, key in [(1.0, "g10"), (1.5, "g15"), (2.0, "g20")]:
        x, F, G, T = acc.ABPG(f, h, L, x0, gamma=gam, maxitrs=N, theta_eq=True, verbose=False)
        assert np.max(np.abs(x - gd["l1_abpg_%s_x" % key])) < 1e-12
        _close(F, gd["l1_abpg_%s_F" % key], 1e-12)
        _close(G[:500], gd["l1_abpg_%s_G" % key][:500], 1e-7)
    x, F, G, T = acc.ABDA(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=True, verbose=False)
    assert np.max(np.abs(x - gd["l1_abda_x"])) < 1e-12
    _close(F, gd["l1_abda_F"], 1e-11)
    x, F, Gamma, G, T = acc.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=N, theta_eq=False, Gmargin=3, verbose=False)
    k = _agree_prefix(Gamma, gd["l1_expo_Gamma"], 1e-12)
    assert k >= 200, k
    _close(F[:k], gd["l1_expo_F"][:k], 1e-6)
    assert abs(F[-1] - gd["l1_expo_F"][-1]) < 1e-6
    x, F, G, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, theta_eq=False, verbose=False)
    k = _agree_prefix(G, gd["l1_gain_G"], 1e-12)
    assert k >= 500, k
    _close(F[:k], gd["l1_gain_F"][:k], 1e-11)
    assert abs(F[-1] - gd["l1_gain_F"][-1]) < 1e-8


def test_poisson_l2_trajectories(acc):
    """ipynb/ex_Poisson_L2.ipynb cell 5 at Poisson_regrL2(100, 1000, noise=1e-3, lamda=1e-3, randseed=1).
    BurgEntropyL2.prox_map evaluates sqrt(gg^2 + 4*lamda_L) - gg with gg ~ 1/y ~ 1e3 and lamda_L ~ 1e-4
    (functions.py:321-323): the subtraction cancels ~10 digits, so the REFERENCE's own prox amplifies a
    1-ulp change of g to ~1e-7 relative in x.  The prox kernel is bit-exact on identical inputs (previous
    tests); trajectories are compared at the level that conditioning allows (measured: x 6e-9, F 4e-9)."""
    gd = golden("poisson")
    f, h, L, x0 = _poisson(acc, "l2")
    N = 2000
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=N, linesearch=False, verbose=False)
    assert np.max(np.abs(x - gd["l2_bpg_x"])) < 5e-7
    _close(F, gd["l2_bpg_F"], 2e-7)
    x, F, G, T = acc.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=False, verbose=False)
    assert np.max(np.abs(x - gd["l2_abpg_x"])) < 5e-7
    _close(F, gd["l2_abpg_F"], 2e-7)
    x, F, Ls, T = acc.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.5, verbose=False)
    k = _agree_prefix(Ls, gd["l2_bpgls_Ls"], 1e-12)
    assert k >= 300, k
    _close(F[:k], gd["l2_bpgls_F"][:k], 2e-7)
    x, F, Gamma, G, T = acc.ABPG_expo(f, h, L, x0, gamma0=3, maxitrs=N, theta_eq=False, Gmargin=1, verbose=False)
    k = _agree_prefix(Gamma, gd["l2_expo_Gamma"], 1e-12)
    assert k >= 300, k
    _close(F[:k], gd["l2_expo_F"][:k], 2e-7)
    x, F, G, Gdiv, Gavg, T = acc.ABPG_gain(f, h, L, x0, gamma=2, maxitrs=N, G0=0.1, ls_inc=1.5, ls_dec=1.5,
                                           theta_eq=True, verbose=False)
    k = _agree_prefix(G, gd["l2_gain_G"], 1e-12)
    assert k >= 300, k
    _close(F[:k], gd["l2_gain_F"][:k], 2e-7)
    assert abs(F[-1] - gd["l2_gain_F"][-1]) < 1e-7


def test_poisson_reference_loop_on_device_objects(acc, O):
    """A NumPy driver loop (the oracle's ABPG) runs unchanged on the device-backed Poisson objects."""
    gd = golden("poisson")
    f, h, L, x0 = _poisson(acc, "l1")
    x, F, G, T = O.ABPG(f, h, L, x0, gamma=2.0, maxitrs=100, theta_eq=True)
    _close(F, gd["l1_abpg_g20_F"][:100], 1e-12)


def test_poisson_large_properties(acc):
    """(8192, 65536), 4 GiB of A: properties that need no CPU pass -- f(x*) = 0 and g(x*) = 0 at a consistent
    x*, directional derivative against a central difference, convexity along a segment."""
    m, n = 8192, 65536
    gen = torch.Generator(device="cuda").manual_seed(3)
    A = torch.rand(m, n, dtype=torch.float64, device="cuda", generator=gen)
    xs = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) / n
    b = A @ xs                                                     # torch: test plumbing only
    f = acc.PoissonRegression(A, b)
    fs, gs = f.func_grad(xs, 2)
    assert abs(fs) < 1e-9 and float(gs.abs().max()) < 1e-7 * float(A.sum(0).max())
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) / n + 1e-6
    d = torch.randn(n, dtype=torch.float64, device="cuda", generator=gen) * 1e-6
    fx, g = f.func_grad(x, 2)
    t = 1e-3
    num = (f(x + t * d) - f(x - t * d)) / (2 * t)
    assert float(g @ d) == pytest.approx(num, rel=1e-6)
    mid = f(0.5 * (x + xs))
    assert mid <= 0.5 * (fx + fs) + 1e-12 and fx > 0
    del A
