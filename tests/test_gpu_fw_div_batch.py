"""Lock-step Bregman-step Frank-Wolfe batches (``D_opt_FW_div_step_batch`` / ``D_opt_FW_descent_step_batch``, C-ABI
``accbpg_dopt_batch_fw_div_probe`` / ``_fw_div_apply``) on the device.  The reference throughout is the sequential
solver on ``batch.instance(i)`` (the batch's own handle and Gram plan): x, F, Ls and the state (x, w, H) must be
BIT-identical -- across the branch points of the kernels, with instances stopping at different iterations, with one
instance at the cap of the step length while its neighbours take rank-one steps, with per-instance refreshes, and at the
edges of the C-ABI (active masks with gaps, an apply that is not the last probe's, batched and single-handle calls
mixed).  tests/fwdiv_numpy.py is compared at the bar of test_gpu_fw_div.py::test_trajectories."""
import ctypes as C

import numpy as np
import pytest

import fwdiv_numpy as R
from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 1e-15
NOOP = (0, 1.0, 0.0, 0.0, 1.0)          # accbpg_fw_update: x * 1, x[0] += 0, H and w: (. + 0 * .) / 1


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _state(batch, i):
    return [t.cpu().numpy() for t in batch.fw_state(i)]


def _batch(acc, m, n, seeds):
    Vs = [gaussian_design(m, n, s) for s in seeds]
    return Vs, acc.DOptimalBatch(Vs)


def _same(res, ref, count=3):
    """x, F, Ls (div step) or x, F (descent) bit for bit, lengths included; the rest has the same length"""
    for a, b in zip(res[:count], ref[:count]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(res[count:], ref[count:]):
        assert len(a) == len(b)


def _both(acc, batch, K, x0, L, iters, same_len=None, **kw):
    """Both solvers on the batch, then the sequential ones on every instance: results and states identical.  Returns the
    two batch results."""
    Lv = np.broadcast_to(np.asarray(L, dtype=np.float64), (K,))
    dkw = {k: v for k, v in kw.items() if k != "linesearch"}
    out = []
    for which in ("div", "descent"):
        if which == "div":
            res = acc.D_opt_FW_div_step_batch(batch, L, x0, iters, 2.0, **kw)
        else:
            res = acc.D_opt_FW_descent_step_batch(batch, x0, iters, **dkw)
        states = [_state(batch, i) for i in range(K)]
        assert len(res) == K
        for i in range(K):
            if which == "div":
                ref = acc.D_opt_FW_div_step(batch.instance(i), float(Lv[i]), x0, iters, 2.0, verbose=False, **kw)
            else:
                ref = acc.D_opt_FW_descent_step(batch.instance(i), x0, iters, verbose=False, **dkw)
            if same_len is not None:
                assert len(ref[1]) == same_len
            _same(res[i], ref, 3 if which == "div" else 2)
            for a, b in zip(states[i], _state(batch, i)):
                np.testing.assert_array_equal(a, b)
        out.append(res)
    return out


# ------------------------------------------------------------------ 1. batch == sequential across the branch points
@pytest.mark.parametrize("m,n,K,iters", [
    (8, 40, 3, 40),
    (37, 203, 3, 40),       # odd m: scalar path of the H kernels; odd n: rows not 16-byte aligned, V pass not vectorised
    (64, 4097, 3, 40),      # past the 1024-entry reduction block and the V pass's column group; last column unpaired
    (128, 2049, 3, 40),     # two reduction blocks and a bit
    (256, 1024, 3, 40),     # several row splits of the pass over V; exactly one reduction block
    (8, 525000, 2, 10),     # past the 512-block cap of the div reductions (512 * 1024 = 524288)
])
def test_batch_equals_sequential(acc, m, n, K, iters):
    Vs, batch = _batch(acc, m, n, [100 + 7 * i + m for i in range(K)])
    x0 = np.ones(n) / n
    div, desc = _both(acc, batch, K, x0, 1.0, iters, same_len=iters)
    assert not np.array_equal(div[0][0], div[1][0])             # (the instances are different problems)
    assert not np.array_equal(desc[0][1], desc[1][1])


# ------------------------------------------------------------------ 2. staggered stops
def _prefix(a, b, tol=1e-12):
    n = min(len(a), len(b))
    bad = np.nonzero(np.abs(a[:n] - b[:n]) > tol * (1 + np.abs(b[:n])))[0]
    return n if bad.size == 0 else int(bad[0])


def test_staggered_stops(acc):
    m, n, maxitrs = 8, 40, 400
    seeds = [301, 302, 303, 304, 305]
    Vs, batch = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    div, desc = _both(acc, batch, len(seeds), x0, 1.0, maxitrs, epsilon=1e-3)
    for name, res in (("div step", div), ("descent", desc)):
        lengths = [len(r[1]) for r in res]
        print(name, "lengths", lengths)
        assert len(set(lengths)) == len(lengths) and max(lengths) < maxitrs
    for i in range(len(seeds)):
        x, F, Ls, _ = div[i]
        xr, Fr, Lsr = R.fw_div_step(Vs[i], 1.0, x0, maxitrs, 2.0, epsilon=1e-3)
        k = _prefix(Ls, Lsr)
        print("div step %d: prefix %d of %d / %d" % (i, k, len(Ls), len(Lsr)))
        assert k >= 150, k
        np.testing.assert_allclose(F[:k], Fr[:k], rtol=1e-9, atol=1e-9)
        x, F, _, _ = desc[i]
        xr, Fr = R.fw_descent_step(Vs[i], x0, maxitrs, epsilon=1e-3)
        assert len(F) == len(Fr)
        np.testing.assert_allclose(F, Fr, rtol=1e-9, atol=1e-9)


# ------------------------------------------------------------------ 3. per-instance L and capped steps
def _capped(acc):
    V = gaussian_design(16, 257, 2)
    return acc.DOptimalBatch([V, V, V]), np.ones(257) / 257, [1.0, 1e-9, 1.0]


def test_rejected_capped_trials_on_one_instance(acc):
    """Instance 1 starts from a tiny L: its first trials sit at the cap a = 1 and are valued in full on its own handle
    (and rejected) while its neighbours accept their first trial; all three share the one apply of the iteration."""
    batch, x0, L = _capped(acc)
    res = acc.D_opt_FW_div_step_batch(batch, L, x0, 12, 2.0)
    states = [_state(batch, i) for i in range(3)]
    assert res[1][2][0] > 1e-6                                  # many doublings in the first iteration
    print("Ls[0] of the three", [r[2][0] for r in res])
    for i in range(3):
        ref = acc.D_opt_FW_div_step(batch.instance(i), L[i], x0, 12, 2.0, verbose=False)
        _same(res[i], ref)
        for a, b in zip(states[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(res[0][1], res[2][1])         # (the same problem with the same L)
    assert not np.array_equal(res[0][2], res[1][2])


def test_accepted_capped_step_on_one_instance(acc):
    """No line search and a tiny L on instance 1: it jumps to the vertex and is re-initialised alone, every iteration,
    while its neighbours step and refresh together.  Should the vertex be singular on the device, the batch raises what
    the sequential solver raises, with the instance named."""
    batch, x0, L = _capped(acc)
    args = dict(linesearch=False, refresh=5)
    try:
        acc.D_opt_FW_div_step(batch.instance(1), L[1], x0, 12, 2.0, verbose=False, **args)
    except ValueError as err:
        print("capped step: the vertex is singular on the device:", err)
        with pytest.raises(ValueError, match="^instance 1: " + str(err)):
            acc.D_opt_FW_div_step_batch(batch, L, x0, 12, 2.0, **args)
        return
    res = acc.D_opt_FW_div_step_batch(batch, L, x0, 12, 2.0, **args)
    states = [_state(batch, i) for i in range(3)]
    print("capped step: F of instance 1", res[1][1][:3])
    assert res[1][1][1] > res[1][1][0] + 100                    # the jump to the vertex
    for i in range(3):
        ref = acc.D_opt_FW_div_step(batch.instance(i), L[i], x0, 12, 2.0, verbose=False, **args)
        _same(res[i], ref)
        for a, b in zip(states[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 4. refresh
def test_refresh(acc):
    m, n, K = 37, 203, 3
    Vs, batch = _batch(acc, m, n, [511, 512, 513])
    x0 = np.ones(n) / n
    _both(acc, batch, K, x0, 1.0, 23, same_len=23, refresh=5)


# ------------------------------------------------------------------ 5. C-ABI edges
def _raw(batch):
    from accbpg_and_fw_amd import _lib
    return _lib, _lib.load(), batch._h


def _ints(vals):
    return (C.c_int * len(vals))(*vals)


def _raw_probe(_lib, lib, h, K, mask, recs=None):
    recs = recs if recs is not None else (_lib.FwDivProbe * K)()
    return lib.accbpg_dopt_batch_fw_div_probe(h, FILL, 1.0, mask, recs), recs


def _raw_apply(lib, h, K, mask, aps):
    p = (C.c_int64 * K)(*[u[0] for u in aps])
    a, hc, hd = [(C.c_double * K)(*[u[j] for u in aps]) for j in (1, 2, 3)]
    return lib.accbpg_dopt_batch_fw_div_apply(h, mask, p, a, FILL, 1.0, hc, hd)


def _scalars(m, rec, a, ld=0.0, q=0.0):
    """(p, a, hcoef, hdiv) of a step of length a towards the vertex of a record"""
    hcoef, hdiv, _, _, _ = R.step_scalars(a, 1.0, dict(w_i=rec.w_i, sum_w=rec.sum_w, sum_u2=rec.sum_u2), ld, q, m)
    return rec.i, a, hcoef, hdiv


def _init(batch, K, n):
    X0 = torch.full((K, n), 1.0 / n, dtype=torch.float64, device="cuda")
    batch.fw_init(X0)


def _unchanged(batch, before, which):
    torch.cuda.synchronize()
    for i in which:
        for a, b in zip(before[i], _state(batch, i)):
            np.testing.assert_array_equal(a, b)


def test_abi_active_mask_bad_pivot_and_moved_state(acc):
    m, n, K = 37, 203, 4
    Vs, batch = _batch(acc, m, n, [601, 602, 603, 604])
    _lib, lib, h = _raw(batch)
    # no Frank-Wolfe state yet: an argument error, not a launch
    rc, recs = _raw_probe(_lib, lib, h, K, None)
    assert rc == _lib.ERR_ARG
    assert _raw_apply(lib, h, K, None, [(0, 0.3, -0.1, 0.7)] * K) == _lib.ERR_ARG
    _init(batch, K, n)
    before = [_state(batch, i) for i in range(K)]
    mask = _ints([1, 0, 1, 0])
    for i in range(K):
        recs[i].i, recs[i].w_i, recs[i].sum_u2 = -7, -7.0, -7.0   # sentinels: records of inactive instances stay unwritten
    rc, recs = _raw_probe(_lib, lib, h, K, mask, recs)
    assert rc == _lib.OK, _lib.last_error()
    for i in (1, 3):
        assert recs[i].i == -7 and recs[i].w_i == -7.0 and recs[i].sum_u2 == -7.0
    for i in (0, 2):
        x, w, H = before[i]
        assert recs[i].i == int(np.argmin(-w)) and recs[i].w_i == w[recs[i].i] and recs[i].min_x == x.min()
        assert recs[i].sum_u2 > 0
    # the record of instance 0 is the one the single-handle probe gives on its handle
    one = _lib.FwDivProbe()
    assert lib.accbpg_fw_div_probe_step(batch.instance(0)._h, FILL, 1.0, C.byref(one)) == _lib.OK
    for name, _ in _lib.FwDivProbe._fields_:
        assert getattr(one, name) == getattr(recs[0], name), name
    aps = [_scalars(m, recs[i], 0.3) if i in (0, 2) else (-1, 0.0, 0.0, 0.0) for i in range(K)]
    # a pivot that is not the last probe's on ONE active instance: refused, no instance moves
    bad = list(aps)
    bad[2] = ((aps[2][0] + 1) % n,) + aps[2][1:]
    assert _raw_apply(lib, h, K, mask, bad) == _lib.ERR_ARG
    assert "instance 2" in _lib.last_error()
    _unchanged(batch, before, range(K))
    # an instance that was not probed (3) in the mask: refused as well
    assert _raw_apply(lib, h, K, _ints([1, 0, 1, 1]), aps) == _lib.ERR_ARG
    _unchanged(batch, before, range(K))
    # (the entries of the INACTIVE instances 1 and 3 are not read)
    assert _raw_apply(lib, h, K, mask, aps) == _lib.OK, _lib.last_error()
    _unchanged(batch, before, (1, 3))
    for i in (0, 2):
        now = _state(batch, i)
        assert all(not np.array_equal(a, b) for a, b in zip(before[i], now))
    # a second apply without a probe in between: refused
    moved = [_state(batch, i) for i in range(K)]
    assert _raw_apply(lib, h, K, mask, aps) == _lib.ERR_ARG
    _unchanged(batch, moved, range(K))
    # an update of the plain kind between the probe and the apply moves the state: refused
    rc, recs = _raw_probe(_lib, lib, h, K, mask, recs)
    assert rc == _lib.OK
    aps = [_scalars(m, recs[i], 0.2) if i in (0, 2) else (-1, 0.0, 0.0, 0.0) for i in range(K)]
    batch.fw_update([True, False, False, False], [NOOP, None, None, None])
    moved = [_state(batch, i) for i in range(K)]
    assert _raw_apply(lib, h, K, mask, aps) == _lib.ERR_ARG
    assert "instance 0" in _lib.last_error()
    _unchanged(batch, moved, range(K))
    assert _raw_apply(lib, h, K, _ints([0, 0, 1, 0]), aps) == _lib.OK      # (instance 2 was not touched: its apply holds)


def _manual(m, n, steps, probe, apply):
    """`steps` iterations of the descent schedule a = 2 / (k + 2) through a probe and an apply callable"""
    for k in range(1, steps + 1):
        rec = probe()
        apply(_scalars(m, rec, 2 / (k + 2)))


def test_abi_batched_and_single_handle_calls_mixed(acc):
    """Ten batched iterations and the eleventh through accbpg_fw_div_probe_step / accbpg_fw_div_apply on instance 0's own
    handle; ten on the handle and the eleventh batched; a twelfth probed on the handle and applied by the batch: each
    equals as many sequential iterations (the step lengths of the descent solver, no refresh)."""
    m, n, K = 64, 4097, 3
    Vs, batch = _batch(acc, m, n, [801, 802, 803])
    _lib, lib, h = _raw(batch)
    x0 = np.ones(n) / n
    h0 = batch.instance(0)._h
    only0 = [True, False, False]

    def single_probe():
        rec = _lib.FwDivProbe()
        assert lib.accbpg_fw_div_probe_step(h0, FILL, 1.0, C.byref(rec)) == _lib.OK
        return rec

    def single_apply(ap):
        assert lib.accbpg_fw_div_apply(h0, ap[0], ap[1], FILL, 1.0, ap[2], ap[3]) == _lib.OK, _lib.last_error()

    def sequential(steps):
        gen = acc.D_opt_alg.D_opt_FW_descent_step_steps(batch.instance(0), x0, steps + 2, verbose=False, refresh=0)
        for _ in range(steps):
            next(gen)
        gen.close()
        return _state(batch, 0)

    # batched, then single
    _init(batch, K, n)
    for k in range(1, 11):
        recs = batch.fw_div_probe()
        batch.fw_div_apply(None, [_scalars(m, recs[i], 2 / (k + 2)) for i in range(K)])
    single_apply(_scalars(m, single_probe(), 2 / 13))
    got = _state(batch, 0)
    for a, b in zip(got, sequential(11)):
        np.testing.assert_array_equal(a, b)
    # single, then batched, then probed on the handle and applied by the batch
    _init(batch, K, n)
    _manual(m, n, 10, single_probe, single_apply)
    recs = batch.fw_div_probe(only0)
    batch.fw_div_apply(only0, [_scalars(m, recs[0], 2 / 13), None, None])
    got = _state(batch, 0)
    for a, b in zip(got, sequential(11)):
        np.testing.assert_array_equal(a, b)
    _init(batch, K, n)
    _manual(m, n, 11, single_probe, single_apply)
    batch.fw_div_apply(only0, [_scalars(m, single_probe(), 2 / 14), None, None])
    got = _state(batch, 0)
    for a, b in zip(got, sequential(12)):
        np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 6. repeatability, tensors stay tensors
def test_two_runs_are_bit_identical_and_tensors_stay_tensors(acc):
    m, n, K = 64, 512, 3
    Vs, batch = _batch(acc, m, n, [901, 902, 903])
    x0 = np.ones(n) / n
    a = acc.D_opt_FW_div_step_batch(batch, [1.0, 0.5, 2.0], x0, 30, 2.0)
    b = acc.D_opt_FW_div_step_batch(batch, [1.0, 0.5, 2.0], x0, 30, 2.0)
    for u, v in zip(a, b):
        _same(u, v)
    a = acc.D_opt_FW_descent_step_batch(batch, x0, 30)
    b = acc.D_opt_FW_descent_step_batch(batch, x0, 30)
    for u, v in zip(a, b):
        _same(u, v, 2)
    X0 = torch.from_numpy(np.tile(x0, (K, 1))).cuda()
    t = acc.D_opt_FW_descent_step_batch(batch, X0, 30)
    for u, v in zip(t, a):
        assert isinstance(u[0], torch.Tensor) and u[0].is_cuda and isinstance(u[1], np.ndarray)
        np.testing.assert_array_equal(u[0].cpu().numpy(), v[0])
        np.testing.assert_array_equal(u[1], v[1])
    t = acc.D_opt_FW_div_step_batch(batch, 1.0, X0[0], 5, 2.0)
    assert all(isinstance(u[0], torch.Tensor) for u in t)
