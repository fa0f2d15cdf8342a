"""``DOptimalBatch.avg_prox`` (C-ABI ``accbpg_dopt_batch_burg_simplex_avg_prox``): ABDA's dual-averaging step of every
active instance in one launch.  Row i of its two outputs equals, bit for bit, what the sequential solver computes with
three launches -- ``vec_axpby(1.0, gavg_i, wgt_i, g_i)``, ``vec_div_scalar(., csum_i)`` and
``BurgEntropySimplex.prox_map(., Lc_i)`` -- and the step counts equal that prox's.  Sizes: the three seams of the
registers-per-thread dispatch (2048, 8192, 32768) from either side, the first long row (32769: the composition itself,
instance by instance), and the smallest rows.  A ``DOptimalBatch`` needs m < n, so the shortest row a batch can have is
n = 2 (with m = 1); the other batches have m = 8."""
import ctypes as C

import numpy as np
import pytest

from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EPS = 1e-8
FILL = -7.25                    # what the outputs hold before a call
SIZES = [2, 63, 1025, 2048, 2049, 8192, 8193, 32768, 32769]
ASSERT_MSG = "BergEntropySimplex prox_map only takes positive L."


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


_BATCHES = {}


def batch_of(acc, n, K):
    if (n, K) not in _BATCHES:
        m = 8 if n > 8 else 1
        _BATCHES[(n, K)] = acc.DOptimalBatch([gaussian_design(m, n, 40 + i) for i in range(K)])
    return _BATCHES[(n, K)]


def operands(n, K, zero_avg, seed=0):
    rng = np.random.RandomState(1000 * K + n + seed)
    G = torch.from_numpy(3.0 * rng.randn(K, n)).cuda()                      # mixed sign
    Gavg = torch.from_numpy(np.zeros((K, n)) if zero_avg else 5.0 * rng.randn(K, n)).cuda()
    theta = 2.0 / (np.arange(K) + 3.0)
    wgt = theta ** (1 - 2.5)                                                # theta^(1 - gamma)
    csum = wgt + (0.0 if zero_avg else 1.0 + rng.rand(K))
    Lc = 1.0 / csum                                                         # L / csum, L = 1
    return Gavg, G, wgt, csum, Lc


def composition(acc, gavg, g, wgt, csum, Lc):
    """What ABDA_steps runs for one instance: (gavg + wgt*g, prox_map(that / csum, Lc), (bisections, Newton steps))."""
    from accbpg_and_fw_amd.functions import vec_axpby, vec_div_scalar
    h = acc.BurgEntropySimplex(EPS)
    a = vec_axpby(1.0, gavg, float(wgt), g)
    z = h.prox_map(vec_div_scalar(a, float(csum)), float(Lc))
    return a.cpu().numpy(), z.cpu().numpy(), h.last_info


def filled(K, n):
    return torch.full((K, n), FILL, dtype=torch.float64, device="cuda")


def check_rows(acc, batch, ops, active):
    Gavg, G, wgt, csum, Lc = ops
    K, n = G.shape
    keep = (Gavg.clone(), G.clone())
    out_avg, out = filled(K, n), filled(K, n)
    ra, rz = batch.avg_prox(Gavg, G, wgt, csum, Lc, EPS, active, out_avg=out_avg, out=out, info=True)
    assert ra is out_avg and rz is out
    assert torch.equal(Gavg.view(torch.int64), keep[0].view(torch.int64))   # the inputs keep their bits
    assert torch.equal(G.view(torch.int64), keep[1].view(torch.int64))
    for i in range(K):
        if active is not None and not active[i]:
            assert bool((out_avg[i] == FILL).all()) and bool((out[i] == FILL).all())
            continue
        a, z, info = composition(acc, Gavg[i], G[i], wgt[i], csum[i], Lc[i])
        np.testing.assert_array_equal(out_avg[i].cpu().numpy(), a)
        np.testing.assert_array_equal(out[i].cpu().numpy(), z)
        assert batch.last_info[i] == info
    return out_avg, out


@pytest.mark.parametrize("zero_avg", [True, False])
@pytest.mark.parametrize("K", [3, 1])
@pytest.mark.parametrize("n", SIZES)
def test_rows_equal_the_sequential_composition(acc, n, K, zero_avg):
    batch = batch_of(acc, n, K)
    ops = operands(n, K, zero_avg)
    active = [True, False, True] if K == 3 else None
    check_rows(acc, batch, ops, active)


def test_allocated_outputs_and_no_info(acc):
    """Without out_avg / out the method allocates them; without `info` nothing is read back -- the same bits."""
    n, K = 2049, 3
    batch = batch_of(acc, n, K)
    Gavg, G, wgt, csum, Lc = operands(n, K, False, seed=3)
    new_avg, Z = batch.avg_prox(Gavg, G, wgt, csum, Lc, EPS)
    for i in range(K):
        a, z, _ = composition(acc, Gavg[i], G[i], wgt[i], csum[i], Lc[i])
        np.testing.assert_array_equal(new_avg[i].cpu().numpy(), a)
        np.testing.assert_array_equal(Z[i].cpu().numpy(), z)


def test_nan_in_g_gives_the_composition_s_nan_pattern(acc):
    n, K = 2049, 3
    batch = batch_of(acc, n, K)
    Gavg, G, wgt, csum, Lc = operands(n, K, False, seed=7)
    G[0, n // 3] = float("nan")
    out_avg, out = check_rows(acc, batch, (Gavg, G, wgt, csum, Lc), None)  # (assert_array_equal: NaN where NaN)
    assert int(torch.isnan(out_avg[0]).sum()) == 1 and not bool(torch.isnan(out_avg[1:]).any())
    assert not bool(torch.isnan(out[1:]).any())


@pytest.mark.parametrize("n", [1025, 32769])
def test_nonpositive_Lc_raises_for_that_instance_only(acc, n):
    K = 3
    batch = batch_of(acc, n, K)
    Gavg, G, wgt, csum, Lc = operands(n, K, False, seed=11)
    Lc = Lc.copy()
    Lc[2] = 0.0
    out_avg, out = filled(K, n), filled(K, n)
    with pytest.raises(AssertionError, match=ASSERT_MSG):
        batch.avg_prox(Gavg, G, wgt, csum, Lc, EPS, None, out_avg=out_avg, out=out)
    for i in (0, 1):
        a, z, _ = composition(acc, Gavg[i], G[i], wgt[i], csum[i], Lc[i])
        np.testing.assert_array_equal(out_avg[i].cpu().numpy(), a)
        np.testing.assert_array_equal(out[i].cpu().numpy(), z)
    assert bool((out_avg[2] == FILL).all()) and bool((out[2] == FILL).all())
    Lc[2] = float("nan")                                                    # not (nan > 0)
    with pytest.raises(AssertionError, match=ASSERT_MSG):
        batch.avg_prox(Gavg, G, wgt, csum, Lc, EPS, None, out_avg=out_avg, out=out)
    check_rows(acc, batch, (Gavg, G, wgt, csum, Lc), [True, True, False])   # ... unless it sits out


def test_in_place_average_and_other_layouts_are_refused(acc):
    from accbpg_and_fw_amd import _lib
    n, K = 1025, 3
    batch = batch_of(acc, n, K)
    Gavg, G, wgt, csum, Lc = operands(n, K, False)
    with pytest.raises(ValueError):
        batch.avg_prox(Gavg, G, wgt, csum, Lc, EPS, out_avg=Gavg)
    # ... by the library too
    vals = [(C.c_double * K)(*v) for v in (wgt, csum, Lc)]
    st = (C.c_int * K)()
    out = filled(K, n)
    P = lambda t: C.c_void_p(t.data_ptr())
    rc = batch._lib.accbpg_dopt_batch_burg_simplex_avg_prox(batch._h, P(Gavg), P(G), n, vals[0], vals[1], vals[2], EPS,
                                                            P(Gavg), P(out), None, st, None)
    assert rc == _lib.ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    wide = torch.zeros(K, n + 1, dtype=torch.float64, device="cuda")
    for bad in (dict(Gavg=wide[:, :n]), dict(G=wide[:, :n]), dict(out=wide[:, :n]), dict(out_avg=wide[:, :n])):
        kw = dict(Gavg=Gavg, G=G)
        kw.update(bad)
        with pytest.raises(ValueError):
            batch.avg_prox(kw.pop("Gavg"), kw.pop("G"), wgt, csum, Lc, EPS, **kw)
