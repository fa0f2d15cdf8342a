"""Lock-step Frank-Wolfe batches (``D_opt_FW_batch`` / ``D_opt_FW_away_batch``, C-ABI ``accbpg_dopt_batch_fw_*``):
instance i of a batch is BIT-identical -- x, F, SP, SN and the state (x, w, H) -- to the sequential solver on
``batch.instance(i)``, across the step kernels' branch points, with instances stopping at different iterations, for
every way F[k] = log det(H_k) is formed, and at the edges of the C-ABI (active masks with gaps, a bad pivot, a singular
instance, batched and single-handle steps mixed)."""
import ctypes as C

import numpy as np
import pytest

from conftest import gaussian_design

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


def _same(res, ref):
    """identical: x, F, SP, SN bit for bit, lengths included (T is wall-clock time)"""
    for a, b in zip(res[:4], ref[:4]):
        np.testing.assert_array_equal(a, b)
    assert len(res[4]) == len(ref[4])


def _state(batch, i):
    return [t.cpu().numpy() for t in batch.fw_state(i)]


def _batch(acc, m, n, seeds):
    Vs = [gaussian_design(m, n, s) for s in seeds]
    return Vs, acc.DOptimalBatch(Vs)


# ------------------------------------------------------------------ 1. batch == sequential across the branch points
@pytest.mark.parametrize("m,n", [
    (8, 40),
    (37, 203),          # odd m: scalar path of the H kernels; odd n: rows not 16-byte aligned, V pass not vectorised
    (64, 4608),         # n >= 4096: two-stage away search; n a multiple of the V pass's column block
    (64, 4097),         # last column unpaired
    (256, 1024),        # a fused-path shape, several row splits
    (16, 140000),       # past the 512-workgroup cap of the fused w-update / probe launch
])
def test_batch_equals_sequential(acc, m, n):
    K, iters = 3, 60
    Vs, batch = _batch(acc, m, n, [100 + 7 * i + m for i in range(K)])
    x0 = np.ones(n) / n
    for solver, bsolver in ((acc.D_opt_FW, acc.D_opt_FW_batch), (acc.D_opt_FW_away, acc.D_opt_FW_away_batch)):
        res = bsolver(batch, x0, -1.0, iters)
        states = [_state(batch, i) for i in range(K)]
        assert len(res) == K
        for i in range(K):
            ref = solver(batch.instance(i), x0, -1.0, iters, verbose=False)
            assert len(ref[1]) == iters
            _same(res[i], ref)
            for a, b in zip(states[i], _state(batch, i)):
                np.testing.assert_array_equal(a, b)
    assert not np.array_equal(res[0][0], res[1][0])             # (the instances are different problems)


# ------------------------------------------------------------------ 2. staggered stopping, away variant
def test_away_staggered_stopping(acc, O):
    m, n, eps, maxitrs = 8, 40, 1e-2, 400
    seeds = [301, 302, 303, 304, 305]
    Vs, batch = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    res = acc.D_opt_FW_away_batch(batch, x0, eps, maxitrs)
    lengths = [len(r[1]) for r in res]
    print("away lengths", lengths)
    assert len(set(lengths)) > 1 and max(lengths) < maxitrs
    for i in range(len(seeds)):
        ref = acc.D_opt_FW_away(batch.instance(i), x0, eps, maxitrs, verbose=False)
        _same(res[i], ref)
        # the oracle, at the bars of test_gpu_parity.test_fw_trajectories
        xo, Fo, SPo, SNo, To = O.D_opt_FW_away(Vs[i], x0, eps, maxitrs)
        x, F, SP, SN, T = res[i]
        assert abs(len(F) - len(Fo)) <= 2
        k = min(len(F), len(Fo))
        assert np.max(np.abs(x - xo)) < 1e-8
        np.testing.assert_allclose(F[:k], Fo[:k], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(SP[:k], SPo[:k], rtol=1e-8, atol=1e-8)


# ------------------------------------------------------------------ 3. stopping, plain variant (by construction)
def test_plain_stop_by_construction(acc):
    """Plain FW from a uniform start never meets its stop test on Gaussian instances (its support never shrinks), so
    instance 1 is built to stop: V = [Q1 | Q2], the Q factors of two Gaussian 8 x 8 matrices side by side, has
    V V^T = 2 I, so with x0 = 1/16 the inverse is H = 8 I and every w_i = 8 |v_i|^2 = 8 = m up to rounding -- both gaps
    are rounding noise and the run stops at k = 0.  (One square Q would give the same H, but a D-optimal objective
    needs m < n -- DOptimalObj and accbpg_dopt_batch_create refuse (8,8) as the reference does -- hence two.)"""
    m, n = 8, 16
    np.random.seed(77)
    Q1, _ = np.linalg.qr(np.random.randn(m, m))
    Q2, _ = np.linalg.qr(np.random.randn(m, m))
    Vs = [gaussian_design(m, n, 41), np.ascontiguousarray(np.hstack([Q1, Q2])), gaussian_design(m, n, 43)]
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    res = acc.D_opt_FW_batch(batch, x0, 1e-6, 50)
    assert len(res[1][1]) == 1 and len(res[1][2]) == 1
    np.testing.assert_array_equal(res[1][0], x0)
    for i in (0, 2):
        assert len(res[i][1]) > 1
        _same(res[i], acc.D_opt_FW(batch.instance(i), x0, 1e-6, 50, verbose=False))


# ------------------------------------------------------------------ 4. the forms of F[k] = log det(H_k)
@pytest.mark.parametrize("kw", [dict(logdet_refresh=0), dict(logdet_refresh=1), dict(logdet_refresh=5), dict()])
def test_logdet_refresh_forms(acc, kw):
    m, n, K, iters = 37, 203, 3, 40
    Vs, batch = _batch(acc, m, n, [511, 512, 513])
    x0 = np.ones(n) / n
    res = acc.D_opt_FW_away_batch(batch, x0, -1.0, iters, **kw)
    for i in range(K):
        ref = acc.D_opt_FW_away(batch.instance(i), x0, -1.0, iters, verbose=False, **kw)
        assert len(ref[1]) == iters and np.all(np.isfinite(ref[1]))
        _same(res[i], ref)


# ------------------------------------------------------------------ 5. C-ABI edges
def _raw(acc, batch):
    from accbpg_and_fw_amd import _lib
    return _lib, _lib.load(), batch._h


def _ints(vals):
    return (C.c_int * len(vals))(*vals)


def _fw_scalars(m, pr):
    """a Frank-Wolfe step's scalars from a probe record (D_opt_alg.py:75-79)"""
    t = (pr.w_i / m - 1) / (pr.w_i - 1)
    coef = t / (1 + t * (pr.w_i - 1))
    return pr.i, 1 - t, t, -coef, 1 - t


def _raw_update(lib, h, K, mask, ups):
    p = (C.c_int64 * K)(*[u[0] for u in ups])
    arrs = [(C.c_double * K)(*[u[j] for u in ups]) for j in range(1, 5)]
    return lib.accbpg_dopt_batch_fw_update(h, mask, p, *arrs)


def test_abi_active_mask_and_bad_pivot(acc):
    m, n, K = 37, 203, 4
    Vs, batch = _batch(acc, m, n, [601, 602, 603, 604])
    _lib, lib, h = _raw(acc, batch)
    X0 = torch.full((K, n), 1.0 / n, dtype=torch.float64, device="cuda")
    batch.fw_init(X0)
    before = [_state(batch, i) for i in range(K)]
    mask = _ints([1, 0, 1, 0])
    probes = (_lib.FwProbe * K)()
    for i in range(K):
        probes[i].i, probes[i].w_i = -7, -7.0                   # sentinels: records of inactive instances stay unwritten
    assert lib.accbpg_dopt_batch_fw_probe(h, 0, mask, probes) == _lib.OK
    for i in (1, 3):
        assert probes[i].i == -7 and probes[i].w_i == -7.0
    for i in (0, 2):
        assert 0 <= probes[i].i < n and probes[i].w_i > m and np.isnan(probes[i].logdet_H)
    ups = [_fw_scalars(m, probes[i]) if i in (0, 2) else (-1, 0.0, 0.0, 0.0, 0.0) for i in range(K)]
    # a pivot outside [0, n) on an ACTIVE instance: refused before anything is launched
    bad = list(ups)
    bad[2] = (n,) + ups[2][1:]
    assert _raw_update(lib, h, K, mask, bad) == _lib.ERR_ARG
    torch.cuda.synchronize()
    for i in range(K):
        for a, b in zip(before[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)
    # (the out-of-range pivots of the INACTIVE instances 1 and 3 are not read)
    assert _raw_update(lib, h, K, mask, ups) == _lib.OK
    for i in (1, 3):
        for a, b in zip(before[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)
    for i in (0, 2):
        assert not np.array_equal(before[i][0], _state(batch, i)[0])
        assert not np.array_equal(before[i][2], _state(batch, i)[2])


def test_abi_singular_instance_at_init(acc):
    """x0 of instance 1 supported on m/2 points: its own status says not positive definite, the others initialise and
    then step exactly as they do alone."""
    m, n, K = 64, 512, 3
    Vs, batch = _batch(acc, m, n, [701, 702, 703])
    _lib, lib, h = _raw(acc, batch)
    X0 = torch.full((K, n), 1.0 / n, dtype=torch.float64, device="cuda")
    X0[1] = 0.0
    X0[1, : m // 2] = 2.0 / m
    st = _ints([-1] * K)
    ld = (C.c_double * K)()
    lib.accbpg_dopt_batch_set_stream(h, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert lib.accbpg_dopt_batch_fw_init(h, C.c_void_p(X0.data_ptr()), n, None, ld, st) == _lib.OK
    assert list(st) == [_lib.OK, _lib.ERR_NOT_PD, _lib.OK]
    mask = [True, False, True]
    steps = 5
    for _ in range(steps):
        prs = batch.fw_probe(0, mask)
        batch.fw_update(mask, [_fw_scalars(m, prs[i]) if mask[i] else None for i in range(K)])
    got = {i: _state(batch, i) for i in (0, 2)}
    # a step on the instance without state is an argument error, not a launch
    probes = (_lib.FwProbe * K)()
    assert lib.accbpg_dopt_batch_fw_probe(h, 0, None, probes) == _lib.ERR_ARG
    x0 = np.ones(n) / n
    for i in (0, 2):
        gen = acc.D_opt_alg.D_opt_FW_steps(batch.instance(i), x0, -1.0, steps + 1, verbose=False)
        for _ in range(steps):
            next(gen)
        for a, b in zip(got[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("away", [0, 1])
def test_abi_single_handle_step_after_batched_steps(acc, away):
    """10 batched steps, then the 11th on instance 0 through accbpg_fw_probe_step / accbpg_fw_update on its own handle
    (the stage-1 records the batched update left are the ones that probe picks up): the state equals that after 11
    sequential steps."""
    m, n, K = 64, 4608, 3
    Vs, batch = _batch(acc, m, n, [801, 802, 803])
    _lib, lib, h = _raw(acc, batch)
    x0 = np.ones(n) / n
    bgen = (acc.D_opt_alg.D_opt_FW_away_batch_steps if away else acc.D_opt_alg.D_opt_FW_batch_steps)(batch, x0, -1.0, 20)
    for _ in range(10):
        next(bgen)
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    h0 = batch.instance(0)._h
    pr = _lib.FwProbe()
    assert lib.accbpg_fw_probe_step(h0, away, 0, C.byref(pr)) == _lib.OK
    if away:
        up = _AwayRun(m, 1, 0, 1).iterate(0, pr, float("nan"), 0.0, 0.0, -1.0)
    else:
        up = (pr.i,) + _fw_decide(m, pr.w_i, pr.w_j, -1.0)[2]
    assert lib.accbpg_fw_update(h0, *up) == _lib.OK
    got = _state(batch, 0)
    sgen = (acc.D_opt_alg.D_opt_FW_away_steps if away else acc.D_opt_alg.D_opt_FW_steps)(
        batch.instance(0), x0, -1.0, 20, verbose=False)
    for _ in range(11):
        next(sgen)
    for a, b in zip(got, _state(batch, 0)):
        np.testing.assert_array_equal(a, b)
    sgen.close()
    bgen.close()
