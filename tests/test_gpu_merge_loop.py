"""The k-loop of the 64x64 tile products (gemm_ops_body: inverse merges, their batched form, Cholesky trailing
updates) keeps the global loads of several k-steps in flight.  It must give the bits of the loop it replaced, which
stays selectable (accbpg_debug_gemm_loop: 0 = production, 1 = one k-step of look-ahead): same MFMAs on the same operands
in the same k order, for every range of k-steps the triangular skips produce -- shorter than the depth, equal to it,
longer, ragged in K, ragged in M and N."""
import numpy as np
import pytest

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


@pytest.fixture(scope="module")
def O():
    from oracle import np_oracle
    return np_oracle


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def under_both_loops(lib, run):
    """run() under switch 0 and under switch 1; the switch is back at 0 afterwards whatever happens"""
    out = []
    try:
        for variant in (0, 1):
            assert lib.accbpg_debug_gemm_loop(variant) == 0
            out.append(run())
    finally:
        lib.accbpg_debug_gemm_loop(0)
    return out


def test_switch_refuses_unknown_variants(lib):
    try:
        assert lib.accbpg_debug_gemm_loop(5) != 0 and lib.accbpg_debug_gemm_loop(-1) != 0
        for v in (1, 2, 3, 4, 0):
            assert lib.accbpg_debug_gemm_loop(v) == 0
    finally:
        lib.accbpg_debug_gemm_loop(0)


@pytest.mark.parametrize("ab", [(-1.0, 0.0), (1.0, 1.0)])
@pytest.mark.parametrize("kmajor", [0, 1])
@pytest.mark.parametrize("MN", [(64, 64), (128, 64), (70, 50)])
@pytest.mark.parametrize("K", [16, 32, 48, 64, 80, 96, 37, 250])
def test_gemm_same_bits_from_both_loops(acc, lib, K, MN, kmajor, ab):
    """1 to 6 k-steps (below, at and above every depth the new loop can be built with) and ragged K, on one tile, two
    tiles and a ragged tile (which takes the guarded loads)."""
    from accbpg_and_fw_amd import _lib
    M, N = MN
    alpha, beta = ab
    rng = np.random.RandomState(1000 * K + 10 * M + N + kmajor)
    A = rng.randn(M, K)
    B = rng.randn(K, N) if kmajor else rng.randn(N, K)
    C0 = rng.randn(M, N)
    Ad, Bd = dev(A), dev(B)

    def run():
        Cd = dev(C0)
        rc = lib.accbpg_test_gemm(Ad.data_ptr(), K, Bd.data_ptr(), B.shape[1], Cd.data_ptr(), N, M, N, K,
                                  kmajor, alpha, beta, 0, None)
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        return Cd.cpu().numpy()

    new, old = under_both_loops(lib, run)
    np.testing.assert_array_equal(new, old)
    Bm = B if kmajor else B.T
    ref = alpha * (A @ Bm) + beta * C0
    scale = np.abs(A) @ np.abs(Bm) + np.abs(C0)
    for got in (new, old):
        assert np.max(np.abs(got - ref) / scale) < 1e-14       # the bound of test_gpu_parity.py's engine test


@pytest.mark.parametrize("m", [64, 128, 192, 200, 320, 512, 576, 1024])
def test_func_grad_same_bits_from_both_loops(acc, lib, O, m):
    """One block and one level (64, 128), ragged last blocks (200), several levels, the first size with a level that
    is split along K (1024) and one where a split level sits beside ragged groups (576).  The gradient is formed from
    the inverse factor the merges leave in the handle, so its agreement with the oracle is the check of W L = I."""
    n = 2 * m
    V = np.random.RandomState(m).randn(m, n)
    rng = np.random.RandomState(m + 1)
    x = rng.rand(n) + 0.01
    x /= x.sum()

    def run():
        f = acc.DOptimalObj(V)
        return f.func_grad(x, 2)

    (f_new, g_new), (f_old, g_old) = under_both_loops(lib, run)
    assert f_new == f_old
    np.testing.assert_array_equal(g_new, g_old)
    fr, gr = O.DOptOracle(V).func_grad(x, 2)
    assert abs(f_new - fr) < 1e-11 * max(1.0, abs(fr))        # the tolerances of test_gpu_parity.py at these shapes
    np.testing.assert_allclose(g_new, gr, rtol=1e-11, atol=0)


def test_batched_merges_same_bits_from_both_loops(acc, lib, O):
    """gemm_ops_batch_kernel: three instances of (256, 512) in one batch."""
    from accbpg_and_fw_amd.batched import DOptimalBatch
    m, n, K = 256, 512, 3
    Vs = [np.random.RandomState(70 + i).randn(m, n) for i in range(K)]
    X = np.random.RandomState(7).rand(K, n) + 0.01
    X /= X.sum(axis=1, keepdims=True)
    Xd = dev(X)

    def run():
        f, G = DOptimalBatch(Vs).func_grad(Xd, 2)
        return f, G.cpu().numpy()

    (f_new, G_new), (f_old, G_old) = under_both_loops(lib, run)
    np.testing.assert_array_equal(f_new, f_old)
    np.testing.assert_array_equal(G_new, G_old)
    for i in range(K):
        fr, gr = O.DOptOracle(Vs[i]).func_grad(X[i], 2)
        assert abs(f_new[i] - fr) < 1e-11 * max(1.0, abs(fr))
        np.testing.assert_allclose(G_new[i], gr, rtol=1e-11, atol=0)
