"""Lock-step Frank-Wolfe batches that decide their steps on the device (``D_opt_FW_batch_device`` /
``D_opt_FW_away_batch_device``, C-ABI ``accbpg_dopt_batch_fw_run``).

The bar throughout is EQUALITY: instance i of a batch -- x, F, SP, SN, the iteration count, the records and the state
(x, w, H) -- against the sequential solver on ``batch.instance(i)``, against ``accbpg_fw_run`` on the instance handles of
a twin batch, and against the lock-step solvers.  The batch-run kernels wrap the bodies of the single handle on its
grids and call its one copy of the device decisions, so there is nothing to tolerate."""
import ctypes as C

import numpy as np
import pytest

from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NAN = float("nan")
APPLIED, STOPPED, BAD_PIVOT, NOT_RUN = 0, 1, 2, 3
FIELDS = ("i", "j", "w_i", "w_j", "x_j", "q_prev", "p", "xscale", "xadd", "hcoef", "hdiv", "kind", "status")


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def L(acc):
    from accbpg_and_fw_amd import _lib
    return _lib


def _same(res, ref, what=""):
    """identical: x, F, SP, SN bit for bit, lengths included (T is wall-clock time)"""
    for a, b in zip(res[:4], ref[:4]):
        np.testing.assert_array_equal(a, b, err_msg=str(what))
    assert len(res[4]) == len(ref[4]), what


def _state(batch, i):
    return [t.cpu().numpy() for t in batch.fw_state(i)]


def _states_equal(a, b, what=""):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v, err_msg=str(what))


def _batch(acc, m, n, seeds):
    Vs = [gaussian_design(m, n, s) for s in seeds]
    return Vs, acc.DOptimalBatch(Vs)


def _init(batch, x0):
    X0 = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(x0, (batch.K, batch.n)))).cuda()
    return batch.fw_init(X0)


def _ints(vals):
    return (C.c_int * len(vals))(*vals)


def _tuples(steps, first, count):
    return [tuple(getattr(steps[first + k], f) for f in FIELDS) for k in range(count)]


def brun(L, batch, away, eps, nsteps, mask=None, sentinel=False):
    """accbpg_dopt_batch_fw_run: (rc, nrun per instance, per instance every record as a tuple in FIELDS order)"""
    K = batch.K
    steps = (L.FwStep * (K * max(nsteps, 1)))()
    if sentinel:
        for s in steps:
            s.i, s.w_i, s.status = -7, -7.0, -7
    nrun = _ints([-7] * K)
    epsv = (C.c_double * K)(*[float(v) for v in np.broadcast_to(eps, (K,))])
    rc = L.load().accbpg_dopt_batch_fw_run(batch._h, int(away), epsv, int(nsteps), None if mask is None else _ints(mask),
                                           steps, nrun)
    return rc, list(nrun), [_tuples(steps, i * nsteps, nsteps) for i in range(K)] if nsteps >= 1 else None


def hrun(L, batch, i, away, eps, nsteps):
    """accbpg_fw_run on the handle of instance i: (rc, nrun, records)"""
    steps = (L.FwStep * nsteps)()
    nrun = C.c_int(-7)
    rc = L.load().accbpg_fw_run(batch.instance(i)._h, int(away), float(eps), int(nsteps), steps, C.byref(nrun))
    return rc, nrun.value, _tuples(steps, 0, nsteps)


def _records_equal(got, want, what):
    """every field (NaN equals NaN)"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for f, a, b in zip(FIELDS, g, w):
            np.testing.assert_array_equal(a, b, err_msg="%s: record %d field %s" % (what, k, f))


# ------------------------------------------------------------------ 1. batch-device == sequential across the branch points
@pytest.mark.parametrize("m,n", [
    (8, 40),
    (37, 203),          # odd m: scalar path of the H kernels; odd n: rows not 16-byte aligned, V pass not vectorised
    (64, 4097),         # n >= 4096: the sliced away search; last column unpaired
    (64, 4608),         # ... n a multiple of the V pass's column block
    (256, 1024),        # several row splits
    (16, 140000),       # past the 512-workgroup cap of the fused w-update / probe launch
])
def test_batch_device_equals_sequential(acc, m, n):
    K, iters = 3, 60
    Vs, batch = _batch(acc, m, n, [100 + 7 * i + m for i in range(K)])
    x0 = np.ones(n) / n
    for solver, bsolver in ((acc.D_opt_FW, acc.D_opt_FW_batch_device), (acc.D_opt_FW_away, acc.D_opt_FW_away_batch_device)):
        runs = []
        for S in (1, 7, 64):
            res = bsolver(batch, x0, -1.0, iters, sync_every=S)
            assert len(res) == K
            runs.append((S, res, [_state(batch, i) for i in range(K)]))
        for i in range(K):
            ref = solver(batch.instance(i), x0, -1.0, iters, verbose=False)
            assert len(ref[1]) == iters
            state = _state(batch, i)
            for S, res, states in runs:
                _same(res[i], ref, (m, n, S, i))
                _states_equal(states[i], state, (m, n, S, i, "state"))
        assert not np.array_equal(runs[0][1][0][0], runs[0][1][1][0])       # (the instances are different problems)


# ------------------------------------------------------------------ 2. staggered stops inside a chunk, away variant
def _spy(batch):
    """log of every fw_run call: (nsteps, active instances, {i: did instance i stop in this call})"""
    log, orig = [], batch.fw_run

    def fw_run(away, eps, nsteps, active=None):
        recs = orig(away, eps, nsteps, active)
        act = [i for i in range(batch.K) if recs[i] is not None]
        log.append((nsteps, act, {i: recs[i][-1].status != APPLIED for i in act}))
        return recs

    batch.fw_run = fw_run
    return log


@pytest.mark.parametrize("kw", [dict(logdet_refresh=0, sync_every=64), dict(logdet_refresh=0, sync_every=7), dict(),
                                dict(sync_every=7)])
def test_away_staggered_stops_inside_a_chunk(acc, kw):
    """The instances of test_gpu_fw_batch.test_away_staggered_stopping (the NumPy oracle stops them at k = 58, 65, 52,
    59, 66).  An instance that stops in mid-call idles through the rest of it while the others run on: every instance
    equals its sequential run, the state of an early stopper -- read after the others have finished -- included."""
    m, n, eps, maxitrs = 8, 40, 1e-2, 400
    seeds = [301, 302, 303, 304, 305]
    Vs, batch = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    log = _spy(batch)
    res = acc.D_opt_FW_away_batch_device(batch, x0, eps, maxitrs, **kw)
    states = [_state(batch, i) for i in range(batch.K)]
    lengths = [len(r[1]) for r in res]
    print("away lengths", lengths, "calls", [(c[0], c[1], sorted(i for i in c[2] if c[2][i])) for c in log])
    assert len(set(lengths)) > 1 and max(lengths) < maxitrs
    # at least one call held both an instance that stopped in it and one that did not
    assert any(any(c[2].values()) and not all(c[2].values()) for c in log)
    # a stopped instance is not in a later call
    gone = set()
    for nsteps, act, stopped in log:
        assert not (gone & set(act))
        gone |= {i for i in act if stopped[i]}
    if kw.get("sync_every") == 64:
        assert len(log) == 2 and log[0][1] == list(range(5)) and sum(log[0][2].values()) == 3 and len(log[1][1]) == 2
    seq_kw = {k: v for k, v in kw.items() if k != "sync_every"}
    for i in range(len(seeds)):
        ref = acc.D_opt_FW_away(batch.instance(i), x0, eps, maxitrs, verbose=False, **seq_kw)
        _same(res[i], ref, (kw, i))
        _states_equal(states[i], _state(batch, i), (kw, i, "state"))


# ------------------------------------------------------------------ 3. a stop at k = 0, plain variant
def test_plain_stop_at_the_start(acc):
    """Instance 1 is the [Q1 | Q2] instance of test_gpu_fw_batch.test_plain_stop_by_construction: every w_i = m up to
    rounding, the run stops at k = 0 and idles through the first chunk of seven beside two running neighbours."""
    m, n = 8, 16
    np.random.seed(77)
    Q1, _ = np.linalg.qr(np.random.randn(m, m))
    Q2, _ = np.linalg.qr(np.random.randn(m, m))
    Vs = [gaussian_design(m, n, 41), np.ascontiguousarray(np.hstack([Q1, Q2])), gaussian_design(m, n, 43)]
    x0 = np.ones(n) / n
    batch = acc.DOptimalBatch(Vs)
    res = acc.D_opt_FW_batch_device(batch, x0, 1e-6, 50, sync_every=7)
    states = [_state(batch, i) for i in range(3)]
    assert len(res[1][1]) == 1 and len(res[1][2]) == 1 and len(res[1][4]) == 1
    np.testing.assert_array_equal(res[1][0], x0)
    np.testing.assert_array_equal(states[1][0], x0)
    for i in (0, 1, 2):
        ref = acc.D_opt_FW(batch.instance(i), x0, 1e-6, 50, verbose=False)
        assert i == 1 or len(ref[1]) > 1
        _same(res[i], ref, i)
        _states_equal(states[i], _state(batch, i), i)


# ------------------------------------------------------------------ 4. the forms of F[k] = log det(H_k)
@pytest.mark.parametrize("kw", [dict(logdet_refresh=0), dict(logdet_refresh=1), dict(logdet_refresh=5), dict()])
def test_logdet_refresh_forms(acc, kw):
    m, n, K, iters = 37, 203, 3, 40
    Vs, batch = _batch(acc, m, n, [511, 512, 513])
    x0 = np.ones(n) / n
    lock = acc.D_opt_FW_away_batch(batch, x0, -1.0, iters, **kw)
    got = {S: acc.D_opt_FW_away_batch_device(batch, x0, -1.0, iters, sync_every=S, **kw) for S in (None, 3)}
    for i in range(K):
        ref = acc.D_opt_FW_away(batch.instance(i), x0, -1.0, iters, verbose=False, **kw)
        assert len(ref[1]) == iters and np.all(np.isfinite(ref[1]))
        for S in (None, 3):
            _same(got[S][i], ref, (kw, S, i))
            _same(got[S][i], lock[i], (kw, S, i, "lock-step"))


# ------------------------------------------------------------------ 5. the records
@pytest.mark.parametrize("m,n", [(37, 203), (16, 4608)])
@pytest.mark.parametrize("away", [0, 1])
def test_records_equal_those_of_the_single_handle(acc, L, m, n, away):
    """accbpg_dopt_batch_fw_run against accbpg_fw_run on the instance handles of a twin batch from the same x0: every
    field of every record, the status-3 tail behind a stop and nrun included, and a call that goes on from a stop."""
    K = 3
    seeds = [900 + m + i for i in range(K)]
    Vs, a = _batch(acc, m, n, seeds)
    _, b = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    _init(a, x0)
    _init(b, x0)
    calls = [(7, [-1.0, -1.0, -1.0]), (9, [-1.0, 1e30, -1.0]), (5, [-1.0, -1.0, 1e30]), (1, [-1.0] * 3), (6, [1e-9] * 3)]
    for c, (nsteps, eps) in enumerate(calls):
        rc, nrun, recs = brun(L, a, away, eps, nsteps)
        assert rc == L.OK, L.last_error()
        for i in range(K):
            rc_h, nrun_h, want = hrun(L, b, i, away, eps[i], nsteps)
            assert rc_h == L.OK and nrun[i] == nrun_h, (c, i, nrun, nrun_h)
            _records_equal(recs[i], want, (m, n, away, c, i))
            _states_equal(_state(a, i), _state(b, i), (m, n, away, c, i))
        if c == 1:
            assert nrun == [9, 1, 9] and [r[-1] for r in recs[1]] == [STOPPED] + [NOT_RUN] * 8
            assert all(r[6] == -1 and r[-2] == -1 for r in recs[1])


# ------------------------------------------------------------------ 6. C-ABI edges
def test_abi_active_mask_with_gaps_and_eps_per_instance(acc, L):
    m, n, K = 37, 203, 4
    seeds = [601, 602, 603, 604]
    Vs, a = _batch(acc, m, n, seeds)
    _, b = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    _init(a, x0)
    _init(b, x0)
    before = [_state(a, i) for i in range(K)]
    eps = [1e-9, NAN, -1.0, NAN]                                # (entries of inactive instances are not read)
    rc, nrun, recs = brun(L, a, 1, eps, 6, mask=[1, 0, 1, 0], sentinel=True)
    assert rc == L.OK, L.last_error()
    for i in (1, 3):
        assert nrun[i] == -7 and all((r[0], r[2], r[-1]) == (-7, -7.0, -7) for r in recs[i])
        _states_equal(before[i], _state(a, i), i)
    for i in (0, 2):
        rc_h, nrun_h, want = hrun(L, b, i, 1, eps[i], 6)
        assert (rc_h, nrun_h, nrun[i]) == (L.OK, 6, 6)
        _records_equal(recs[i], want, i)
        _states_equal(_state(a, i), _state(b, i), i)
    # an empty active set launches nothing
    rc, nrun, recs = brun(L, a, 1, eps, 6, mask=[0, 0, 0, 0], sentinel=True)
    assert rc == L.OK and nrun == [-7] * K


def test_abi_arguments(acc, L):
    m, n, K = 8, 40, 3
    Vs, batch = _batch(acc, m, n, [611, 612, 613])
    # no instance has Frank-Wolfe state yet
    rc, nrun, recs = brun(L, batch, 0, -1.0, 4, sentinel=True)
    assert rc == L.ERR_ARG and nrun == [-7] * K
    X0 = torch.full((K, n), 1.0 / n, dtype=torch.float64, device="cuda")
    batch.fw_init(X0, active=[True, False, True])
    before = [_state(batch, i) for i in (0, 2)]
    # instance 1 has none: refused before anything is launched, and named
    rc, nrun, recs = brun(L, batch, 0, -1.0, 4, sentinel=True)
    assert rc == L.ERR_ARG and "instance 1" in L.last_error() and nrun == [-7] * K
    assert all(r[-1] == -7 for i in range(K) for r in recs[i])
    for bad in (0, -1, 1025):
        assert brun(L, batch, 0, -1.0, bad, mask=[1, 0, 1])[0] == L.ERR_ARG
    with pytest.raises(ValueError):
        batch.fw_run(0, -1.0, 1025, [True, False, True])
    torch.cuda.synchronize()
    for i, st in zip((0, 2), before):
        _states_equal(st, _state(batch, i), i)
    # the most one call holds
    rc, nrun, recs = brun(L, batch, 0, -1.0, 1024, mask=[1, 0, 1])
    assert rc == L.OK and nrun[0] == 1024 and nrun[2] == 1024 and recs[2][-1][-1] == APPLIED
    out = batch.fw_run(0, [-1.0, 0.0, 1e30], 3, [True, False, True])
    assert out[1] is None and len(out[0]) == 3 and len(out[2]) == 1 and out[2][0].status == STOPPED


def _host_update(L, batch, away, mask):
    """one lock-step probe / update pair with the host's decisions (never a stop: eps = -1)"""
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    prs = batch.fw_probe(away, mask)
    ups = [None] * batch.K
    for i in range(batch.K):
        if not mask[i]:
            continue
        if away:
            ups[i] = _AwayRun(batch.m, 1, 0, 1).iterate(0, prs[i], NAN, 0.0, 0.0, -1.0)
        else:
            ups[i] = (prs[i].i,) + _fw_decide(batch.m, prs[i].w_i, prs[i].w_j, -1.0)[2]
    batch.fw_update(mask, ups)


@pytest.mark.parametrize("m,n", [(37, 203), (16, 4608)])
@pytest.mark.parametrize("away", [0, 1])
def test_abi_mixed_with_the_other_step_calls(acc, L, m, n, away):
    """accbpg_dopt_batch_fw_run between lock-step probe / update pairs and single-handle accbpg_fw_run calls on one
    instance, in both orders, against the same numbers of iterations by accbpg_fw_run alone on a twin batch: the
    stage-1 records an update leaves for the next probe, and their bookkeeping, pass between the interfaces."""
    K = 3
    seeds = [950 + m + i for i in range(K)]
    Vs, a = _batch(acc, m, n, seeds)
    _, b = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    _init(a, x0)
    _init(b, x0)
    every = [True] * K
    done = [0] * K

    def batch_run(nsteps, mask=None):
        rc, nrun, recs = brun(L, a, away, -1.0, nsteps, mask=mask)
        assert rc == L.OK, L.last_error()
        for i in range(K):
            if mask is None or mask[i]:
                assert nrun[i] == nsteps
                done[i] += nsteps

    def pairs(count, mask):
        for _ in range(count):
            _host_update(L, a, away, mask)
        for i in range(K):
            done[i] += count if mask[i] else 0

    def single(i, nsteps):
        rc, nrun, recs = hrun(L, a, i, away, -1.0, nsteps)
        assert (rc, nrun) == (L.OK, nsteps)
        done[i] += nsteps

    pairs(2, every)                 # update -> batch run: instance-wide stage-1 records waiting
    batch_run(5)
    pairs(2, [True, False, True])   # batch run -> probe; instance 1 keeps its waiting records, the others get new ones
    batch_run(4)
    single(1, 3)                    # batch run -> single-handle run
    batch_run(4)                    # single-handle run -> batch run
    a.fw_probe(1 - away, [False, False, True])      # a probe with the other threshold: instance 2 has no records waiting
    batch_run(3)                    # ... and gets the fresh stage 1 beside two that do not
    single(0, 2)
    batch_run(2, mask=[1, 1, 0])
    assert done == [24, 23, 20]
    for i in range(K):
        rc, nrun, recs = hrun(L, b, i, away, -1.0, done[i])
        assert (rc, nrun) == (L.OK, done[i])
        _states_equal(_state(a, i), _state(b, i), (m, n, away, i))
    # what the next probe reads is the same, too
    pa, pb = a.fw_probe(away), None
    for i in range(K):
        pb = L.FwProbe()
        assert L.load().accbpg_fw_probe_step(b.instance(i)._h, away, 0, C.byref(pb)) == L.OK
        assert (pa[i].i, pa[i].j) == (pb.i, pb.j)
        np.testing.assert_array_equal([pa[i].w_i, pa[i].w_j, pa[i].x_j, pa[i].q_prev], [pb.w_i, pb.w_j, pb.x_j, pb.q_prev])


def test_abi_the_largest_batch(acc):
    """K = ACCBPG_BATCH_MAX = 64 instances of (8, 40): the active set, the per-instance nblk of the first iteration and
    eps travel by value in the kernel arguments and must fit their limit at the largest batch; every position of the
    tables is used (first, middle, last checked against the sequential solver)."""
    m, n, K, iters = 8, 40, 64, 20
    Vs, batch = _batch(acc, m, n, [2000 + i for i in range(K)])
    x0 = np.ones(n) / n
    eps = [-1.0] * K
    eps[31] = -2.0                                              # (one per instance)
    fw = acc.D_opt_FW_batch_device(batch, x0, eps, iters, sync_every=7)
    fw_states = {i: _state(batch, i) for i in (0, 31, 63)}
    away = acc.D_opt_FW_away_batch_device(batch, x0, eps, iters)
    away_states = {i: _state(batch, i) for i in (0, 31, 63)}
    assert len(fw) == K and len(away) == K
    for i in (0, 31, 63):
        _same(fw[i], acc.D_opt_FW(batch.instance(i), x0, eps[i], iters, verbose=False), i)
        _states_equal(fw_states[i], _state(batch, i), i)
        _same(away[i], acc.D_opt_FW_away(batch.instance(i), x0, eps[i], iters, verbose=False), i)
        _states_equal(away_states[i], _state(batch, i), i)
    assert all(len(r[1]) == iters for r in fw + away)


# ------------------------------------------------------------------ 7. a NaN in one instance's w
@pytest.mark.parametrize("n", [203, 4097])
@pytest.mark.parametrize("away", [0, 1])
def test_nan_in_one_instance(acc, L, n, away):
    """w of instance 1 all NaN (an update with hcoef = NaN, as test_gpu_fw_device plants it): neither the stop test nor
    eps_pos >= eps_neg holds for a NaN, so with eps = 1e30 it takes the steps the single handle takes, while the
    neighbours, with their own eps, run as they do alone."""
    m, K = 16, 3
    seeds = [970 + i for i in range(K)]
    Vs, a = _batch(acc, m, n, seeds)
    _, b = _batch(acc, m, n, seeds)
    _, clean = _batch(acc, m, n, seeds)
    x0 = np.ones(n) / n
    for bt in (a, b, clean):
        _init(bt, x0)
    for bt in (a, b):
        assert L.load().accbpg_fw_update(bt.instance(1)._h, 5, 1.0, 0.0, NAN, 1.0) == L.OK
    assert np.all(np.isnan(_state(a, 1)[1]))
    eps = [-1.0, 1e30, -1.0]
    for c, nsteps in enumerate((3, 2)):
        rc, nrun, recs = brun(L, a, away, eps, nsteps)
        assert rc == L.OK and nrun == [nsteps] * K, L.last_error()
        for i in range(K):
            rc_h, nrun_h, want = hrun(L, (b if i == 1 else clean), i, away, eps[i], nsteps)
            assert (rc_h, nrun_h) == (L.OK, nsteps)
            _records_equal(recs[i], want, (n, away, c, i))
            _states_equal(_state(a, i), _state((b if i == 1 else clean), i), (n, away, c, i))
        if c == 0:
            r = recs[1][0]
            assert np.isnan(r[2]) and r[-1] == APPLIED and r[-2] == (1 if away else 0)
    for i in (0, 2):
        assert np.all(np.isfinite(_state(a, i)[1]))
