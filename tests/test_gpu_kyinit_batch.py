"""GPU tests of the batched Kumar-Yildirim start (accbpg_dopt_batch_kyinit, DOptimalBatch.kyinit_picks,
D_opt_KYinit_batch).

The contract is free of tolerance: instance i of the batched call is bit for bit accbpg_dopt_kyinit on
accbpg_dopt_batch_instance(b, i) -- `picked` equal step by step, Q equal bit for bit -- and therefore bit for bit the
NumPy restatement tests/ky_numpy.py given that instance's own accbpg_dopt_vt_times as the pass over V.  Every instance
has its own V and its own B, so a swapped table entry shows.

The comparison with the host D_opt_KYinit holds only where no decision is within rounding of a tie; it is made on the
instance sets whose smallest gaps tests/test_kyinit_batch_cpu.py pins (>= 3.8e-6)."""
import ctypes as C

import numpy as np
import pytest

import ky_numpy
from conftest import gaussian_design
from test_kyinit_batch_cpu import SETS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

# (m, n, K): smallest sizes | wave seam of the dots | 256-thread seam | arg-extremum one-block / two-block seam at 1024
# entries (1025: odd n, the scalar-load path of the pass over V) | the 128-record cap | general
SHAPES = [(1, 3, 2), (2, 5, 3), (63, 200, 2), (64, 200, 2), (65, 200, 3), (257, 2100, 2), (8, 1024, 2), (8, 1025, 2),
          (8, 132100, 2), (130, 1030, 5)]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _data(m, n, i):
    rng = np.random.RandomState(1000 * m + n + i)
    return rng.randn(m, n), rng.rand(m, m)


def _check(picked, Q, rp, rQ, what):
    bad = np.nonzero(picked != rp)[0]
    assert bad.size == 0, "%s: first differing pick at step %d (%s): batch %d, other %d" % (
        what, bad[0] // 2, "kmin" if bad[0] & 1 else "kmax", picked[bad[0]], rp[bad[0]])
    np.testing.assert_array_equal(Q, rQ, err_msg=what)


def _run(batch, Bs):
    """the batched call: picked (K x 2m) and, per instance, Q with column j = direction j"""
    K, m = batch.K, batch.m
    Qd = torch.full((K, m, m), float("nan"), dtype=torch.float64, device="cuda")
    picked = batch.kyinit_picks(np.stack(Bs), Q_out=Qd)
    assert picked.shape == (K, 2 * m) and picked.dtype == np.int64
    Q = Qd.cpu().numpy()
    return picked, [Q[i].T for i in range(K)]


def _replay(batch, i, V, B):
    f = batch.instance(i)
    return ky_numpy.kyinit(V, B, vt_times=lambda q: f.vt_times(q).cpu().numpy())[:2]


def _single(batch, i, B):
    m = batch.m
    Qd = torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda")
    picked = batch.instance(i).kyinit_picks(B, Q_out=Qd)
    return picked, Qd.cpu().numpy().T


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


# ------------------------------------------------------------------ 1. replay and single-call equality
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_every_instance_equals_its_replay_and_its_single_call(acc, shape):
    m, n, K = shape
    data = [_data(m, n, i) for i in range(K)]
    batch = acc.DOptimalBatch([V for V, _ in data])
    picked, Q = _run(batch, [B for _, B in data])
    for i, (V, B) in enumerate(data):
        _check(picked[i], Q[i], *_replay(batch, i, V, B), what="instance %d against its replay" % i)
        _check(picked[i], Q[i], *_single(batch, i, B), what="instance %d against its single call" % i)
        assert np.all(np.isfinite(Q[i]))


# ------------------------------------------------------------------ 2. batch sizes
@pytest.mark.parametrize("K", [1, 64])
def test_batch_sizes(acc, K):
    """one instance, and ACCBPG_BATCH_MAX of them"""
    m, n = 16, 600
    data = [_data(m, n, i) for i in range(K)]
    batch = acc.DOptimalBatch([V for V, _ in data])
    picked, Q = _run(batch, [B for _, B in data])
    for i, (V, B) in enumerate(data):
        _check(picked[i], Q[i], *_single(batch, i, B), what="instance %d against its single call" % i)
    if K > 1:
        assert not np.array_equal(picked[0], picked[1])         # (the instances are different problems)


# ------------------------------------------------------------------ 3. padded rows, through the C-ABI
def test_padded_rows_through_the_c_abi(acc):
    """ldv = n + 5 with the padding full of NaN, which must never be read"""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n, K, pad = 33, 777, 2, 5
    data = [_data(m, n, i) for i in range(K)]
    stores = []
    for V, _ in data:
        store = torch.full((m, n + pad), float("nan"), dtype=torch.float64, device="cuda")
        store[:, :n] = torch.from_numpy(V).cuda()
        stores.append(store)
    ptrs = (C.c_void_p * K)(*[s.data_ptr() for s in stores])
    b = C.c_void_p()
    assert lib.accbpg_dopt_batch_create(ptrs, K, m, n, n + pad, None, C.byref(b)) == _lib.OK, _lib.last_error()
    try:
        Bd = torch.from_numpy(np.stack([B for _, B in data])).cuda()
        Qd = torch.full((K, m, m), float("nan"), dtype=torch.float64, device="cuda")
        picked = np.full((K, 2 * m), -1, dtype=np.int64)
        rc = lib.accbpg_dopt_batch_kyinit(b, C.c_void_p(Bd.data_ptr()), picked.ctypes.data_as(C.POINTER(C.c_int64)),
                                          C.c_void_p(Qd.data_ptr()))
        assert rc == _lib.OK, _lib.last_error()
        Q = Qd.cpu().numpy()
        for i, (V, B) in enumerate(data):
            h = C.c_void_p(lib.accbpg_dopt_batch_instance(b, i))

            def vt_times(q, h=h):
                qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
                u = torch.empty(n, dtype=torch.float64, device="cuda")
                assert lib.accbpg_dopt_vt_times(h, C.c_void_p(qd.data_ptr()), C.c_void_p(u.data_ptr())) == _lib.OK
                torch.cuda.synchronize()
                return u.cpu().numpy()
            rp, rQ = ky_numpy.kyinit(V, B, vt_times=vt_times)[:2]
            _check(picked[i], Q[i].T, rp, rQ, what="instance %d against its replay" % i)
            assert np.all(np.isfinite(Q[i]))
    finally:
        lib.accbpg_dopt_batch_destroy(b)


# ------------------------------------------------------------------ 4. planted ties beside a plain instance
def test_planted_ties_beside_a_plain_instance(acc):
    """instances 0 and 1 hold every column twice (as halves, interleaved): each arg-extremum is an exact tie and the
    first index must win at every stage of the merge, while instance 2 beside them is an ordinary problem"""
    m, n0 = 16, 1030
    (V0, B0), (V1, B1) = _data(m, n0, 0), _data(m, n0, 1)
    V2, B2 = _data(m, 2 * n0, 2)
    Vs = [np.ascontiguousarray(np.concatenate([V0, V0], axis=1)), np.ascontiguousarray(np.repeat(V1, 2, axis=1)), V2]
    Bs = [B0, B1, B2]
    batch = acc.DOptimalBatch(Vs)
    picked, Q = _run(batch, Bs)
    assert np.all(picked[0] < n0)
    assert np.all(picked[1] % 2 == 0)
    for i in range(3):
        _check(picked[i], Q[i], *_replay(batch, i, Vs[i], Bs[i]), what="instance %d against its replay" % i)


# ------------------------------------------------------------------ 5. state is left alone
def test_state_is_left_alone(acc):
    m, n, K = 30, 1000, 3
    data = [_data(m, n, i) for i in range(K)]
    Vs, Bs = [V for V, _ in data], np.stack([B for _, B in data])
    batch = acc.DOptimalBatch(Vs)
    X = torch.from_numpy(np.random.RandomState(2).rand(K, n)).cuda()
    X = (X / X.sum(dim=1, keepdim=True)).contiguous()
    f0, G0 = batch.func_grad(X, 2)
    Q1 = torch.full((K, m, m), float("nan"), dtype=torch.float64, device="cuda")
    Q2 = torch.full((K, m, m), float("nan"), dtype=torch.float64, device="cuda")
    p1 = batch.kyinit_picks(Bs, Q_out=Q1)
    f1, G1 = batch.func_grad(X, 2)
    np.testing.assert_array_equal(f1, f0)
    assert torch.equal(G1, G0)
    p2 = batch.kyinit_picks(Bs, Q_out=Q2)                       # two calls in a row
    p3 = batch.kyinit_picks(torch.from_numpy(Bs).cuda())        # a device tensor, the call's own Q
    np.testing.assert_array_equal(p1, p2)
    np.testing.assert_array_equal(p1, p3)
    assert torch.equal(Q1, Q2)

    # a lock-step solver interrupted after three steps goes on as if nothing had happened
    x0, eps, iters = np.ones(n) / n, -1.0, 12
    want = acc.D_opt_FW_away_batch(batch, x0, eps, iters)
    gen = acc.D_opt_alg.D_opt_FW_away_batch_steps(batch, x0, eps, iters)
    for _ in range(3):
        next(gen)
    np.testing.assert_array_equal(batch.kyinit_picks(Bs), p1)
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            got = stop.value
            break
    assert len(got) == K
    for res, ref in zip(got, want):
        for a, b in zip(res[:4], ref[:4]):                      # x, F, SP, SN (T is wall-clock time)
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 6. end to end
@pytest.fixture(scope="module")
def starts(acc):
    """per set: the batch, the batched starts under np.random.seed(rs), the loop of device starts and the loop of host
    starts under the same seed, and the generator after each"""
    out = {}
    for m, n, seeds, rs, _ in SETS:
        Vs = [gaussian_design(m, n, seed) for seed in seeds]    # (built first: gaussian_design reseeds the generator)
        batch = acc.DOptimalBatch(Vs)
        np.random.seed(rs)
        X0, picked = acc.D_opt_KYinit_batch(batch, return_picked=True)
        s_batch = np.random.get_state()
        np.random.seed(rs)
        x_dev = np.stack([acc.D_opt_KYinit_device(batch.instance(i)) for i in range(len(seeds))])
        s_dev = np.random.get_state()
        np.random.seed(rs)
        x_host = np.stack([acc.D_opt_KYinit(batch.instance(i)) for i in range(len(seeds))])
        s_host = np.random.get_state()
        out[(m, n)] = dict(Vs=Vs, batch=batch, X0=X0, picked=picked, x_dev=x_dev, x_host=x_host, s_batch=s_batch,
                           s_dev=s_dev, s_host=s_host, rs=rs)
    return out


@pytest.mark.parametrize("case", SETS, ids=lambda t: "%dx%dx%d" % (t[0], t[1], len(t[2])))
def test_batched_start_equals_the_loop_of_device_starts_and_of_host_starts(acc, starts, case):
    m, n, seeds = case[:3]
    c = starts[(m, n)]
    assert c["X0"].shape == (len(seeds), n) and isinstance(c["X0"], np.ndarray)
    np.testing.assert_array_equal(c["X0"], c["x_dev"])
    assert _same_state(c["s_batch"], c["s_dev"])
    np.testing.assert_array_equal(c["X0"], c["x_host"])
    assert _same_state(c["s_batch"], c["s_host"])
    assert c["picked"].shape == (len(seeds), 2 * m)
    for i in range(len(seeds)):
        np.testing.assert_array_equal(c["X0"][i], ky_numpy.x0_from_picked(c["picked"][i], n))


def test_batched_start_from_matrices_and_into_fw_away_batch(acc, starts):
    c = starts[(30, 1000)]
    np.random.seed(c["rs"])
    np.testing.assert_array_equal(acc.D_opt_KYinit_batch(c["Vs"]), c["X0"])     # a sequence of matrices, too
    batch, X0 = c["batch"], c["X0"]
    res = acc.D_opt_FW_away_batch(batch, X0, 1e-8, 200)
    assert len(res) == batch.K
    for i in range(batch.K):
        ref = acc.D_opt_FW_away(batch.instance(i), X0[i], 1e-8, 200, verbose=False)
        for a, b in zip(res[i][:4], ref[:4]):                   # x, F, SP, SN
            np.testing.assert_array_equal(a, b)


# ------------------------------------------------------------------ 7. arguments
def test_arguments_are_checked(acc, starts):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    batch = starts[(30, 1000)]["batch"]
    K, m = batch.K, batch.m
    B = torch.zeros((K, m, m), dtype=torch.float64, device="cuda")
    picked = (C.c_int64 * (K * 2 * m))()
    assert lib.accbpg_dopt_batch_kyinit(None, C.c_void_p(B.data_ptr()), picked, None) == _lib.ERR_ARG
    assert lib.accbpg_dopt_batch_kyinit(batch._h, None, picked, None) == _lib.ERR_ARG
    assert lib.accbpg_dopt_batch_kyinit(batch._h, C.c_void_p(B.data_ptr()), None, None) == _lib.ERR_ARG
    with pytest.raises(AssertionError):
        batch.kyinit_picks(np.zeros((K, m, m + 1)))
    with pytest.raises(AssertionError):
        batch.kyinit_picks(np.zeros((K + 1, m, m)))
    Qt = torch.empty((K, m, m), dtype=torch.float64, device="cuda").transpose(1, 2)
    assert not Qt.is_contiguous()
    with pytest.raises(AssertionError):
        batch.kyinit_picks(np.zeros((K, m, m)), Q_out=Qt)
