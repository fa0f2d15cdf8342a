"""The lock-step Bregman-step batches with the line search predicted on the device (D_opt_FW_div_step_batch_device,
D_opt_FW_descent_step_batch_device) and their C-ABI call accbpg_dopt_batch_fw_div_run.

The contract is equality bit for bit, no tolerance anywhere: the solvers against D_opt_FW_div_step /
D_opt_FW_descent_step on ``batch.instance(i)`` -- x, F, Ls / G, the iteration count and the state (x, w, H) -- for both
``replay`` values, and the C call against accbpg_fw_div_run on the instance handles of a twin batch: every record byte
for byte, nrun and the state.  ``stats`` is printed, and asserted only where a roll-back or a hand-back was planted.

Shapes are those at which the kernels change form: (8,40); (37,203) -- odd m, rows not 16-byte aligned, at the C level
also with padded rows (ldv 208, and the odd 205, the padding NaN); (64,4097) and (128,2049) past one reduction block;
(256,1024) with several row splits of the pass over V; (8,525000) past the 512-block cap, at K = 2 and a few iterations."""
import ctypes as C

import numpy as np
import pytest

from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 1e-15
NAN = float("nan")
SHAPES = [(8, 40, 3, 40), (37, 203, 3, 40), (64, 4097, 3, 40), (128, 2049, 3, 40), (256, 1024, 3, 40), (8, 525000, 2, 6)]


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


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _state(batch, i):
    return [t.cpu().numpy() for t in batch.fw_state(i)]


def _same_result(got, want, count, what):
    assert len(got[1]) == len(want[1]), (what, len(got[1]), len(want[1]))
    for j in range(count):
        assert np.array_equal(_bits(got[j]), _bits(want[j])), (what, j)
    for a, b in zip(got[count:], want[count:]):
        assert len(a) == len(b), what


_batches = {}
_refs = {}


def _batch(acc, m, n, K, seed0=None):
    key = (m, n, K, seed0)
    if key not in _batches:
        seeds = [(100 + m if seed0 is None else seed0) + 7 * i for i in range(K)]
        _batches[key] = acc.DOptimalBatch([gaussian_design(m, n, s) for s in seeds])
    return _batches[key]


def _reference(acc, batch, key, which, Lv, x0, iters, gamma=2.0, **kw):
    """The sequential solver on every instance handle and the state it leaves: once per argument set, left unchanged."""
    key = (key, which, tuple(np.atleast_1d(Lv)), iters, gamma, tuple(sorted(kw.items())))
    if key not in _refs:
        out = []
        Ls = np.broadcast_to(np.asarray(Lv, dtype=np.float64), (batch.K,))
        for i in range(batch.K):
            if which == "div":
                r = acc.D_opt_FW_div_step(batch.instance(i), float(Ls[i]), x0, iters, gamma, verbose=False, **kw)
            else:
                r = acc.D_opt_FW_descent_step(batch.instance(i), x0, iters, verbose=False, **kw)
            out.append((r, _state(batch, i)))
        _refs[key] = out
    return _refs[key]


def _check(acc, batch, key, which, Lv, x0, iters, S, replay, gamma=2.0, stats=None, **kw):
    dkw = {k: v for k, v in kw.items() if k not in ("linesearch", "ls_ratio")}
    want = _reference(acc, batch, key, which, Lv, x0, iters, gamma, **(kw if which == "div" else dkw))
    stats = {} if stats is None else stats
    if which == "div":
        got = acc.D_opt_FW_div_step_batch_device(batch, Lv, x0, iters, gamma, sync_every=S, stats=stats, replay=replay, **kw)
    else:
        got = acc.D_opt_FW_descent_step_batch_device(batch, x0, iters, sync_every=S, stats=stats, replay=replay, **dkw)
    assert len(got) == batch.K
    for i in range(batch.K):
        what = (key, which, S, replay, i)
        _same_result(got[i], want[i][0], 3 if which == "div" else 2, what)
        if which == "descent":
            assert np.array_equal(got[i][3], want[i][0][3]), what
        for name, a, b in zip("xwH", _state(batch, i), want[i][1]):
            assert np.array_equal(_bits(a), _bits(b)), (what, name)
    return got, stats


# ---- solver against solver -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,K,iters", SHAPES)
def test_solvers_equal_the_sequential_solvers(acc, m, n, K, iters):
    batch = _batch(acc, m, n, K)
    x0 = np.ones(n) / n
    for which in ("div", "descent"):
        for S in (1, 7, 64):
            for replay in ("c", "python"):
                got, stats = _check(acc, batch, (m, n), which, 1.0, x0, iters, S, replay)
                print(which, (m, n), "S", S, replay, [len(g[1]) for g in got], stats)
    assert not np.array_equal(got[0][0], got[1][0])              # (the instances are different problems)


@pytest.mark.parametrize("kw", [dict(refresh=0), dict(refresh=5), dict(refresh=256), dict(ls_ratio=1.5), dict(radius=2.5),
                                dict(linesearch=False), dict(radius=2.5, refresh=5, ls_ratio=1.5)],
                         ids=lambda d: ",".join("%s=%s" % kv for kv in d.items()))
def test_variants_and_per_instance_L(acc, kw):
    batch = _batch(acc, 30, 1000, 3)
    x0 = np.ones(1000) / 1000
    for which in ("div", "descent"):
        for S in (7, 64):
            for replay in ("c", "python"):
                got, stats = _check(acc, batch, (30, 1000), which, [1.0, 3.0, 0.25], x0, 60, S, replay, **kw)
                print(which, kw, "S", S, replay, stats)


def test_other_gamma(acc):
    """The step length itself goes through pow: roll-backs are natural; only identity is asserted."""
    batch = _batch(acc, 16, 257, 3)
    x0 = np.ones(257) / 257
    for replay in ("c", "python"):
        got, stats = _check(acc, batch, (16, 257), "div", 1.0, x0, 120, 16, replay, gamma=1.5)
        print("gamma 1.5", replay, stats)


def test_generator_names_and_replay_argument(acc):
    from accbpg_and_fw_amd import D_opt_alg as D
    batch = _batch(acc, 8, 40, 3)
    x0 = np.ones(40) / 40
    ks = list(D.D_opt_FW_div_step_batch_device_steps(batch, 1.0, x0, 20, 2.0, sync_every=7))
    assert ks == sorted(ks) and ks[-1] == 19, ks
    ks = list(D.D_opt_FW_descent_step_batch_device_steps(batch, x0, 20, sync_every=7))
    assert ks == sorted(ks) and ks[-1] == 19, ks
    with pytest.raises(ValueError, match="replay"):
        acc.D_opt_FW_div_step_batch_device(batch, 1.0, x0, 20, 2.0, replay="numpy")
    with pytest.raises(ValueError, match="sync_every"):
        acc.D_opt_FW_div_step_batch_device(batch, 1.0, x0, 20, 2.0, sync_every=0)


# ---- stops, hand-backs, roll-backs ---------------------------------------------------------------------------------
def test_staggered_stops_inside_a_chunk(acc):
    """Five instances that stop at different iterations of ONE chunk (no refresh, sync_every = maxitrs): an early
    stopper idles through the rest of the call and its state, read at the end, is the sequential solver's."""
    batch = _batch(acc, 8, 40, 5, seed0=301)
    x0 = np.ones(40) / 40
    for which in ("div", "descent"):
        for replay in ("c", "python"):
            got, stats = _check(acc, batch, "stops", which, 1.0, x0, 400, 400, replay, epsilon=1e-3, refresh=0)
            lengths = [len(g[1]) for g in got]
            print(which, replay, "lengths", lengths, stats)
            assert len(set(lengths)) >= 3 and max(lengths) < 400


def test_stop_at_the_first_iteration(acc):
    batch = _batch(acc, 8, 40, 3)
    x0 = np.ones(40) / 40
    for which in ("div", "descent"):
        for replay in ("c", "python"):
            got, stats = _check(acc, batch, "first", which, 1.0, x0, 30, 7, replay, epsilon=float("inf"))
            assert [len(g[1]) for g in got] == [2, 2, 2]        # (k > 0 in the div step's test; F[1] - F[0] in the other)


def test_one_instance_at_the_cap_while_the_others_run_on(acc):
    V = gaussian_design(16, 257, 2)
    batch = acc.DOptimalBatch([V, V, V])
    x0 = np.ones(257) / 257
    for kw in (dict(), dict(linesearch=False)):
        for replay in ("c", "python"):
            got, stats = _check(acc, batch, "cap", "div", [1.0, 1e-9, 1.0], x0, 40, 7, replay, **kw)
            print("capped", kw, replay, stats)
            assert stats["handed_back"] >= 1
            assert np.array_equal(got[0][0], got[2][0]) and not np.array_equal(got[0][0], got[1][0])


@pytest.mark.parametrize("which,field", [("div", "a"), ("div", "hcoef"), ("div", "L"), ("div", "status"),
                                         ("descent", "a"), ("descent", "hdiv"), ("descent", "status")])
@pytest.mark.parametrize("replay", ["c", "python"])
def test_tampered_record_rolls_one_instance_back(acc, monkeypatch, which, field, replay):
    """One field of record 3 of instance 1 of the second chunk is changed between the C call and the replay: that
    instance alone is restored, the results stay identical and the count is the baseline's plus one."""
    batch = _batch(acc, 30, 1000, 3)
    x0 = np.ones(1000) / 1000
    _, base = _check(acc, batch, (30, 1000), which, [1.0, 3.0, 0.25], x0, 60, 7, replay)
    real, calls, restored = batch.fw_div_run, [], []

    def tampering(mode, params, nsteps, active=None, radius=1):
        out = real(mode, params, nsteps, active, radius)
        calls.append(nsteps)
        if len(calls) == 2:
            r = out[1].array[out[1].first + 3]
            if field == "status":
                r.status = 1 - r.status
            else:
                setattr(r, field, float(np.nextafter(getattr(r, field), np.inf)))
        return out
    monkeypatch.setattr(batch, "fw_div_run", tampering)
    monkeypatch.setattr(batch, "fw_restore", lambda i, real=batch.fw_restore: (restored.append(i), real(i))[1])
    got, stats = _check(acc, batch, (30, 1000), which, [1.0, 3.0, 0.25], x0, 60, 7, replay)
    print(which, field, replay, stats, "restored", restored)
    assert stats["rollbacks"] == base["rollbacks"] + 1 == len(restored) and 1 in restored
    assert stats["handed_back"] == base["handed_back"]
    if base["rollbacks"] == 0:
        assert restored == [1]                                  # that instance alone


@pytest.mark.parametrize("planted", [(0,), (10,), (13,), (7, 8)], ids=str)
def test_perturbed_host_scalars_roll_back(acc, monkeypatch, planted):
    """_DivBook.scalars of the HOST refuses the first three trials of the planted iterations, on every instance, as
    test_gpu_fw_div_device.py does for one handle.  The patch is of the Python text, so the replay is the Python one;
    every planted iteration of every instance is rolled back, and no other (the unperturbed run has none)."""
    from accbpg_and_fw_amd import D_opt_alg as D
    batch = _batch(acc, 30, 1000, 3)
    x0 = np.ones(1000) / 1000
    _, base = _check(acc, batch, (30, 1000), "div", 1.0, x0, 40, 7, "python")
    real, realdecide = D._DivBook.scalars, D._DivStepRun.decide

    def scalars(self, a, rec):
        hcoef, hdiv, ld1, q1, f1 = real(self, a, rec)
        if self.iteration in planted and self.refused < 3:
            self.refused += 1
            f1 = float("inf")
        return hcoef, hdiv, ld1, q1, f1

    def decide(self, k, rec, now, capped):
        self.book.iteration, self.book.refused = k, 0
        return realdecide(self, k, rec, now, capped)
    monkeypatch.setattr(D._DivBook, "scalars", scalars)
    monkeypatch.setattr(D._DivStepRun, "decide", decide)
    got, stats = _check(acc, batch, ("perturbed", planted), "div", 1.0, x0, 40, 7, "python")
    print("planted", planted, stats)
    assert stats["rollbacks"] == base["rollbacks"] + 3 * len(planted)


# ---- the C level: a batch against single-handle calls on the instance handles of a twin batch ------------------------
class CBatch:
    """K instances made through the C-ABI on matrices with row stride ``ldv`` (the padding holds NaN)."""

    def __init__(self, L, Vs, ldv=None):
        self.L, self.lib = L, L.load()
        self.K = len(Vs)
        self.m, self.n = Vs[0].shape
        ldv = self.n if ldv is None else ldv
        self.bufs = []
        for V in Vs:
            buf = torch.full((self.m, ldv), NAN, dtype=torch.float64, device="cuda")
            buf[:, :self.n] = torch.from_numpy(np.ascontiguousarray(V))
            self.bufs.append(buf)
        ptrs = (C.c_void_p * self.K)(*[b.data_ptr() for b in self.bufs])
        self.b = C.c_void_p()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.accbpg_dopt_batch_create(ptrs, self.K, self.m, self.n, ldv, stream, C.byref(self.b))
        assert rc == L.OK, L.last_error()
        self.h = [C.c_void_p(self.lib.accbpg_dopt_batch_instance(self.b, i)) for i in range(self.K)]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.accbpg_dopt_batch_destroy(self.b)

    def mask(self, active):
        return None if active is None else (C.c_int * self.K)(*[1 if a else 0 for a in active])

    def init(self, x0, active=None):
        X = torch.from_numpy(np.tile(x0, (self.K, 1))).cuda()
        ld, st = (C.c_double * self.K)(), (C.c_int * self.K)()
        rc = self.lib.accbpg_dopt_batch_fw_init(self.b, C.c_void_p(X.data_ptr()), self.n, self.mask(active), ld, st)
        assert rc == self.L.OK and not any(st), self.L.last_error()
        return list(ld)

    def state(self, i):
        x = torch.empty(self.n, dtype=torch.float64, device="cuda")
        w = torch.empty(self.n, dtype=torch.float64, device="cuda")
        H = torch.empty(self.m, self.m, dtype=torch.float64, device="cuda")
        rc = self.lib.accbpg_fw_get_state(self.h[i], *[C.c_void_p(t.data_ptr()) for t in (x, w, H)])
        assert rc == self.L.OK, self.L.last_error()
        return [t.cpu().numpy() for t in (x, w, H)]

    def set_state(self, i, x, w, H):
        ts = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (x, w, H)]
        assert self.lib.accbpg_fw_set_state(self.h[i], *[C.c_void_p(t.data_ptr()) for t in ts]) == self.L.OK
        torch.cuda.synchronize()

    def params(self, mode, books, gamma=2.0, ls_ratio=2.0, eps=1e-14):
        """books[i] = (k0, L, ld, q, F_prev) or None"""
        prm = (self.L.FwDivParams * self.K)()
        for i, bk in enumerate(books):
            if bk is not None:
                k0, Lc, ld, q, F_prev = bk
                prm[i] = self.L.FwDivParams(mode, 0, k0, Lc, gamma, ls_ratio, eps, ld, q, F_prev)
        return prm

    def run(self, prm, nsteps, active=None, value=1.0, steps=None, nrun=None):
        steps = (self.L.FwDivStep * (self.K * self.L.FW_RUN_MAX))() if steps is None else steps
        nrun = (C.c_int * self.K)(*([-7] * self.K)) if nrun is None else nrun
        rc = self.lib.accbpg_dopt_batch_fw_div_run(self.b, FILL, float(value), prm, nsteps, self.mask(active), steps, nrun)
        return rc, steps, nrun

    def run_single(self, i, prm, nsteps, value=1.0):
        steps = (self.L.FwDivStep * nsteps)()
        nrun = C.c_int(-7)
        rc = self.lib.accbpg_fw_div_run(self.h[i], FILL, float(value), C.byref(prm[i]), nsteps, steps, C.byref(nrun))
        return rc, steps, nrun.value

    def probe(self, i, value=1.0):
        rec = self.L.FwDivProbe()
        rc = self.lib.accbpg_fw_div_probe_step(self.h[i], FILL, float(value), C.byref(rec))
        assert rc == self.L.OK, self.L.last_error()
        return rec

    def apply(self, i, p, a, hcoef, hdiv, value=1.0):
        return self.lib.accbpg_fw_div_apply(self.h[i], int(p), float(a), FILL, float(value), float(hcoef), float(hdiv))


def _twin_states_equal(a, b, what, which=None):
    for i in (range(a.K) if which is None else which):
        for name, u, v in zip("xwH", a.state(i), b.state(i)):
            assert np.array_equal(_bits(u), _bits(v)), (what, i, name)


def _records_equal(a, b, prm, nsteps, what, active=None, value=1.0):
    """The batched call on ``a``, accbpg_fw_div_run on every active instance handle of ``b``: byte for byte."""
    rc, steps, nrun = a.run(prm, nsteps, active, value)
    out = []
    for i in range(a.K):
        if active is not None and not active[i]:
            continue
        rcs, single, n1 = b.run_single(i, prm, nsteps, value)
        assert nrun[i] == n1, (what, i, nrun[i], n1)
        for j in range(nsteps):
            assert bytes(steps[i * a.L.FW_RUN_MAX + j]) == bytes(single[j]), (what, i, j)
        out.append(rcs)
    assert (rc == a.L.OK) == all(r == a.L.OK for r in out), (what, rc, out)
    _twin_states_equal(a, b, what)
    return steps, nrun


def _designs(m, n, K):
    return [gaussian_design(m, n, 900 + m + 3 * i) for i in range(K)]


@pytest.mark.parametrize("m,n,ldv,K,chunks", [(37, 203, 208, 3, (1, 7, 23)), (37, 203, 205, 3, (1, 7, 23)),
                                              (64, 4097, None, 3, (7, 23)), (256, 1024, None, 2, (7,)),
                                              (8, 525000, None, 2, (3,))], ids=str)
def test_call_equals_the_single_handle_call(L, m, n, ldv, K, chunks):
    Vs = _designs(m, n, K)
    x0 = np.ones(n) / n
    with CBatch(L, Vs, ldv) as a, CBatch(L, Vs, ldv) as b:
        ld = a.init(x0)
        assert b.init(x0) == ld
        books = [(2 * i, 1.0 + i, ld[i], 0.0, 0.0) for i in range(K)]          # per-instance k0 and L
        for chunk in chunks:
            steps, nrun = _records_equal(a, b, a.params(L.FW_DIV_LINESEARCH, books), chunk, ("div", chunk))
            assert list(nrun) == [chunk] * K
            last = [steps[i * L.FW_RUN_MAX + chunk - 1] for i in range(K)]
            books = [(books[i][0] + chunk, last[i].L, last[i].ld1, last[i].q1, 0.0) for i in range(K)]
        for i in range(K):                                      # the classical step from here: a probe pending on both
            a.probe(i), b.probe(i)
        cl = [(bk[0] + 1, 0.0, bk[2], bk[3], 1e300) for bk in books]
        steps, nrun = _records_equal(a, b, a.params(L.FW_DIV_CLASSICAL, cl), min(chunks[-1], 9), "classical")
        assert all(steps[i * L.FW_RUN_MAX].a == 2 / (cl[i][0] + 2) for i in range(K))
        for i in range(K):                                      # ... and what the call leaves pending takes an apply
            r = steps[i * L.FW_RUN_MAX + nrun[i] - 1]
            assert a.apply(i, r.probe.i, 0.25, -0.01, 0.75) == L.OK and b.apply(i, r.probe.i, 0.25, -0.01, 0.75) == L.OK
        _twin_states_equal(a, b, "apply behind the classical call")


def test_stops_and_hand_backs_in_mid_call(L):
    """Instance 0 stops at its record 1 (epsilon = inf), instance 1 is handed back at once (a fixed tiny L: the cap),
    instance 2 runs on: the records behind a stop read "not run" and the three states are the single handle's."""
    Vs = _designs(16, 257, 3)
    x0 = np.ones(257) / 257
    with CBatch(L, Vs) as a, CBatch(L, Vs) as b:
        ld = a.init(x0)
        b.init(x0)
        prm = a.params(L.FW_DIV_FIXED_L, [(0, 1.0, ld[0], 0.0, 0.0), (0, 1e-12, ld[1], 0.0, 0.0), (0, 1.0, ld[2], 0.0, 0.0)])
        prm[0].epsilon = float("inf")
        steps, nrun = _records_equal(a, b, prm, 6, "stop / hand-back / run")
        status = [[steps[i * L.FW_RUN_MAX + j].status for j in range(6)] for i in range(3)]
        assert status == [[0, 1, 3, 3, 3, 3], [2, 3, 3, 3, 3, 3], [0] * 6] and list(nrun) == [2, 1, 6]
        assert steps[L.FW_RUN_MAX].reason == L.FW_DIV_HB_CAP
        for i in range(3):                                      # what each instance has pending is the single handle's
            ra, rb = a.probe(i), b.probe(i)
            assert bytes(ra) == bytes(rb), i


def test_masks_with_gaps_leave_the_other_rows_alone(L):
    Vs = _designs(8, 40, 4)
    x0 = np.ones(40) / 40
    with CBatch(L, Vs) as a, CBatch(L, Vs) as b:
        ld = a.init(x0)
        b.init(x0)
        active = [True, False, True, False]
        steps = (L.FwDivStep * (4 * L.FW_RUN_MAX))()
        C.memset(steps, 0xAB, C.sizeof(steps))
        nrun = (C.c_int * 4)(-7, -7, -7, -7)
        prm = a.params(L.FW_DIV_LINESEARCH, [(0, 1.0, ld[i], 0.0, 0.0) if active[i] else None for i in range(4)])
        prm[1].mode = prm[3].mode = 9                           # (entries of inactive instances are not read)
        rc, steps, nrun = a.run(prm, 5, active, steps=steps, nrun=nrun)
        assert rc == L.OK and list(nrun) == [5, -7, 5, -7]
        raw = bytes(steps)
        size, row = C.sizeof(L.FwDivStep), C.sizeof(L.FwDivStep) * L.FW_RUN_MAX
        for i in range(4):
            untouched = raw[i * row + (5 * size if active[i] else 0):(i + 1) * row]
            assert untouched == b"\xab" * len(untouched), i
        for i in (0, 2):
            rcs, single, n1 = b.run_single(i, prm, 5)
            assert rcs == L.OK and all(bytes(steps[i * L.FW_RUN_MAX + j]) == bytes(single[j]) for j in range(5))
        _twin_states_equal(a, b, "mask", (0, 2))
        for i in (1, 3):                                        # the inactive instances did not move
            assert np.array_equal(a.state(i)[0], x0)


def test_argument_errors_move_no_instance(L):
    Vs = _designs(8, 40, 3)
    x0 = np.ones(40) / 40
    with CBatch(L, Vs) as a:
        prm = a.params(L.FW_DIV_LINESEARCH, [(0, 1.0, 0.0, 0.0, 0.0)] * 3)
        assert a.run(prm, 4)[0] == L.ERR_ARG                    # no instance has Frank-Wolfe state
        ld = a.init(x0, [True, True, False])
        assert a.run(prm, 4)[0] == L.ERR_ARG and "instance 2" in L.last_error()      # ... one has none
        a.init(x0)
        before = [a.state(i) for i in range(3)]
        steps, nrun = (L.FwDivStep * (3 * L.FW_RUN_MAX))(), (C.c_int * 3)()
        call = a.lib.accbpg_dopt_batch_fw_div_run
        assert call(a.b, FILL, 1.0, prm, 0, None, steps, nrun) == L.ERR_ARG
        assert call(a.b, FILL, 1.0, prm, L.FW_RUN_MAX + 1, None, steps, nrun) == L.ERR_ARG
        assert call(a.b, FILL, 1.0, None, 4, None, steps, nrun) == L.ERR_ARG
        assert call(a.b, FILL, 1.0, prm, 4, None, None, nrun) == L.ERR_ARG
        assert call(a.b, FILL, 1.0, prm, 4, None, steps, None) == L.ERR_ARG
        prm[1].mode = L.FW_DIV_FIXED_L                          # mixed modes
        assert a.run(prm, 4)[0] == L.ERR_ARG and "mode" in L.last_error()
        prm[1].mode = 3
        assert a.run(prm, 4)[0] == L.ERR_ARG
        cl = a.params(L.FW_DIV_CLASSICAL, [(1, 0.0, 0.0, 0.0, 0.0)] * 3)
        a.probe(0), a.probe(2)                                  # instance 1 has no probe pending
        assert a.run(cl, 4)[0] == L.ERR_ARG and "pending" in L.last_error() and "instance 1" in L.last_error()
        for i in range(3):
            for u, v in zip(a.state(i), before[i]):
                assert np.array_equal(_bits(u), _bits(v)), i
        # nothing was disturbed: the pending probes still take their apply, and a run goes through
        r = a.probe(0)
        assert a.apply(0, r.i, 0.2, -0.2 / (0.8 + 0.2 * r.w_i), 0.8) == L.OK
        assert a.run(a.params(L.FW_DIV_LINESEARCH, [(0, 1.0, ld[0], 0.0, 0.0)] * 3), 4)[0] == L.OK


@pytest.mark.parametrize("order", ["brun-steps-single-brun", "steps-fwrun-brun-steps", "single-brun-fwrun-brun-single"])
def test_mixing(L, order):
    """The new call interleaved with the batched probe / apply, accbpg_fw_div_run on the instance handles and
    accbpg_dopt_batch_fw_run: batch a follows ``order``, its twin does everything with single-handle calls."""
    K, n = 3, 512
    Vs = _designs(64, n, K)
    x0 = np.ones(n) / n
    with CBatch(L, Vs) as a, CBatch(L, Vs) as b:
        ld = a.init(x0)
        b.init(x0)
        books = [(0, 1.0, ld[i], 0.0, 0.0) for i in range(K)]

        def advance(last, count):
            for i in range(K):
                r = last(i)
                books[i] = (books[i][0] + count, r.L, r.ld1, r.q1, 0.0)

        def brun():
            steps, nrun = _records_equal(a, b, a.params(L.FW_DIV_LINESEARCH, books), 5, (order, "brun"))
            advance(lambda i: steps[i * L.FW_RUN_MAX + 4], 5)

        def single():
            prm = a.params(L.FW_DIV_LINESEARCH, books)
            rows = []
            for i in range(K):
                ra, rb = a.run_single(i, prm, 4), b.run_single(i, prm, 4)
                assert ra[0] == rb[0] == L.OK and all(bytes(ra[1][j]) == bytes(rb[1][j]) for j in range(4))
                rows.append(ra[1])
            advance(lambda i: rows[i][3], 4)

        def steps():
            probes = (L.FwDivProbe * K)()
            assert a.lib.accbpg_dopt_batch_fw_div_probe(a.b, FILL, 1.0, None, probes) == L.OK
            p, av, hc, hd = (C.c_int64 * K)(), (C.c_double * K)(), (C.c_double * K)(), (C.c_double * K)()
            for i in range(K):
                assert bytes(b.probe(i)) == bytes(probes[i]), (order, i)
                p[i], av[i], hc[i], hd[i] = probes[i].i, 0.2, -0.2 / (0.8 + 0.2 * probes[i].w_i), 0.8
                assert b.apply(i, p[i], av[i], hc[i], hd[i]) == L.OK
            assert a.lib.accbpg_dopt_batch_fw_div_apply(a.b, None, p, av, FILL, 1.0, hc, hd) == L.OK

        def fwrun():
            eps = (C.c_double * K)(*([1e-9] * K))
            rows, nrun = (L.FwStep * (K * 2))(), (C.c_int * K)()
            assert a.lib.accbpg_dopt_batch_fw_run(a.b, 0, eps, 2, None, rows, nrun) == L.OK
            for i in range(K):
                one, n1 = (L.FwStep * 2)(), C.c_int()
                assert b.lib.accbpg_fw_run(b.h[i], 0, 1e-9, 2, one, C.byref(n1)) == L.OK
                assert n1.value == nrun[i] and bytes(one) == bytes(rows[2 * i]) + bytes(rows[2 * i + 1])

        for word in order.split("-"):
            {"brun": brun, "single": single, "steps": steps, "fwrun": fwrun}[word]()
            _twin_states_equal(a, b, (order, word))


def test_full_batch_of_64_and_a_nan_in_one_w(acc, L):
    """K = ACCBPG_BATCH_MAX: the by-value kernel arguments at their largest.  Then a NaN in the w of instance 5: its
    records (a NaN pivot value, the hand-back or the steps that follow) are the single handle's, the others run on."""
    K, n = 64, 40
    Vs = [gaussian_design(8, n, 2000 + i) for i in range(K)]
    x0 = np.ones(n) / n
    with CBatch(L, Vs) as a, CBatch(L, Vs) as b:
        ld = a.init(x0)
        b.init(x0)
        books = [(i % 3, 1.0, ld[i], 0.0, 0.0) for i in range(K)]
        steps, nrun = _records_equal(a, b, a.params(L.FW_DIV_LINESEARCH, books), 6, "K = 64")
        assert list(nrun) == [6] * K
        for t in (a, b):
            x, w, H = t.state(5)
            w[7] = NAN
            t.set_state(5, x, w, H)
        books = [(6, steps[i * L.FW_RUN_MAX + 5].L, steps[i * L.FW_RUN_MAX + 5].ld1, steps[i * L.FW_RUN_MAX + 5].q1, 0.0)
                 for i in range(K)]
        steps, nrun = _records_equal(a, b, a.params(L.FW_DIV_LINESEARCH, books), 4, "NaN in w")
        r = steps[5 * L.FW_RUN_MAX]
        print("NaN in w: record 0 of instance 5: i %d status %d reason %d, nrun %d" % (r.probe.i, r.status, r.reason, nrun[5]))
        assert r.probe.i == 7 and r.probe.w_i != r.probe.w_i and all(nrun[i] == 4 for i in range(K) if i != 5)
    batch = acc.DOptimalBatch(Vs)
    got, stats = _check(acc, batch, "K64", "div", 1.0, x0, 20, 7, "c")
    print("K = 64 solver", stats)
