"""ABPG_gain enqueues a whole line-search trial through accbpg_dopt_burg_trial and waits for it once
(include/accbpg_hip.h, DOptimalObj.one_wait_trials): the launches are those of the stepwise calls, so nothing the solver
returns may change by a bit, a trial that is not clean commits nothing, and the F[k] lookup inside the trial keeps the
guards of the stepwise lookup.  Shapes: (300, 3000) small tile, one-launch Cholesky, ragged last block, prox <8>;
(1536, 4096) big tile, the side handle factors in small launches; (64, 33024) multi-workgroup prox inside a trial."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [((300, 3000), 60), ((1536, 4096), 30), ((64, 33024), 30)]
REPLAY = 5


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def lib():
    from accbpg_and_fw_amd import _lib
    return _lib.load()


_DESIGNS = {}


def design(m, n):
    """One Gaussian design per shape on the device, shared by the tests (never written to)."""
    if (m, n) not in _DESIGNS:
        gen = torch.Generator(device="cuda").manual_seed(1000 * m + n)
        _DESIGNS[(m, n)] = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    return _DESIGNS[(m, n)]


def point(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    return x / x.sum()


def stats(lib, h):
    cmp_, ans = C.c_int64(0), C.c_int64(0)
    assert lib.accbpg_dopt_value_reuse_stats(h, C.byref(cmp_), C.byref(ans)) == 0
    return cmp_.value, ans.value


def ptr(t):
    return C.c_void_p(t.data_ptr())


def workspace(lib, n):
    return torch.empty(lib.accbpg_vec_workspace_doubles(n), dtype=torch.float64, device="cuda")


def c_trial(lib, h, x_prev, z_prev, theta, L, want_fk, eps=1e-8):
    """accbpg_dopt_burg_trial on the default stream -> (rc, (y, g, z, x), TrialOut)."""
    from accbpg_and_fw_amd import _lib
    n = x_prev.numel()
    vecs = tuple(torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(4))
    out = _lib.TrialOut()
    torch.cuda.synchronize()
    rc = lib.accbpg_dopt_burg_trial(h, ptr(x_prev), ptr(z_prev), theta, L, eps, want_fk, *[ptr(v) for v in vecs],
                                    ptr(workspace(lib, n)), C.byref(out))
    return rc, vecs, out


# ------------------------------------------------------------------ 1. traces
_RUNS = {}


def solve(acc, shape, iters, mode, one_wait, reuse=True, f=None):
    """ABPG_gain from the uniform start -> (its tuple, oracle calls, values reused, trials through the entry); computed
    once per setting and shared (never written to)."""
    key = (shape, iters, mode, one_wait, reuse)
    if f is None and key in _RUNS:
        return _RUNS[key]
    V = design(*shape)
    if f is None:
        f = acc.DOptimalObj(V)
    f.one_wait_trials(one_wait)
    f.reuse_values(reuse)
    if mode == "serial":
        f.overlap_values(False)
    elif mode == "profile":
        f.profile(True)
    h = acc.BurgEntropySimplex()
    x0 = (1.0 / V.shape[1]) * np.ones(V.shape[1])
    calls0, reused0, trials0 = dict(f.calls), f.values_reused, f.one_wait_trials_run
    out = acc.ABPG_gain(f, h, 1.0, x0, gamma=2, maxitrs=iters, verbose=False)
    res = (out, {k: f.calls[k] - calls0[k] for k in calls0}, f.values_reused - reused0, f.one_wait_trials_run - trials0)
    _RUNS.setdefault(key, res)
    return res


def same_traces(a, b):
    assert len(a) == len(b) == 6
    for u, v in zip(a[:-1], b[:-1]):                            # (T, the wall-clock stamps, is last)
        np.testing.assert_array_equal(u, v)


@pytest.mark.parametrize("mode", ["overlap", "serial", "profile"])
@pytest.mark.parametrize("shape,iters", SHAPES)
def test_abpg_gain_traces_do_not_change(acc, shape, iters, mode):
    """Every array ABPG_gain returns except T, the oracle-call counts and the number of values answered from the record
    are the same with the stepwise loop and with one-wait trials: F[k] on the side stream, on the solver's stream, and
    with kernel timing on (the benchmark's timed region)."""
    off, calls_off, reused_off, trials_off = solve(acc, shape, iters, mode, False)
    on, calls_on, reused_on, trials_on = solve(acc, shape, iters, mode, True)
    same_traces(off, on)
    F, Gain = on[1], on[2]
    assert len(F) == iters                                      # (no early stop: the counts below mean something)
    assert calls_off == calls_on
    assert reused_off == reused_on == len(F) - 1
    assert trials_off == 0
    # the gain is cut by 1.2 before every search and raised by 1.2 per failed trial: a gain that did not fall failed once
    failed = int(np.sum(Gain[1:] > Gain[:-1] / 1.2 * 1.1))
    print("shape", shape, "mode", mode, "iterations with a failed trial:", failed, "trials through the entry:", trials_on)
    assert failed >= 1                                          # (the iteration counts reach the retry regime)
    assert trials_on == calls_on["grad"]                        # every trial went through the entry, none was replayed
    assert trials_on >= iters + failed


# ------------------------------------------------------------------ 2. one trial against the stepwise calls
@pytest.mark.parametrize("theta", [1.0, 0.3])
@pytest.mark.parametrize("shape", [s for s, _ in SHAPES])
def test_one_trial_equals_the_stepwise_calls(acc, lib, shape, theta):
    m, n = shape
    V = design(m, n)
    f, f2 = acc.DOptimalObj(V), acc.DOptimalObj(V)
    if theta == 1.0:                                            # the first iteration: x_prev and z_prev are the start
        x_prev = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
        z_prev = x_prev.clone()
    else:
        x_prev, z_prev = point(n, 21), point(n, 22)
    L = theta ** (2 - 1) * (1.0 / 1.2) * 1.0
    fk = f(x_prev)                                              # leaves the record the trial's lookup answers from
    rc, (y, g, z, x), out = c_trial(lib, f._h, x_prev, z_prev, theta, L, 1)
    assert rc == 0
    state = (C.c_int * 3)()
    assert lib.accbpg_debug_prox_state(state) == 0
    assert (state[0], state[1]) == ((2, 5) if n > 32768 else (11, 1))       # the form the dispatch picks for this n

    ws = workspace(lib, n)
    y2, g2, z2, x2 = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(4))
    fy, fx = C.c_double(), C.c_double()
    info = (C.c_int * 2)()
    terms = (C.c_double * 3)()
    assert lib.accbpg_vec_axpby(1.0 - theta, ptr(x_prev), theta, ptr(z_prev), n, ptr(y2), None) == 0
    assert lib.accbpg_dopt_func_grad(f2._h, ptr(y2), 2, C.byref(fy), ptr(g2)) == 0
    assert lib.accbpg_burg_simplex_div_prox(ptr(z_prev), ptr(g2), L, 1e-8, n, ptr(z2), ptr(ws), info, None) == 0
    assert lib.accbpg_vec_axpby(1.0 - theta, ptr(x_prev), theta, ptr(z2), n, ptr(x2), None) == 0
    assert lib.accbpg_ls_terms(ptr(g2), ptr(x2), ptr(y2), ptr(z2), ptr(z_prev), n, terms, ptr(ws), None) == 0
    assert lib.accbpg_dopt_func_grad(f2._h, ptr(x2), 0, C.byref(fx), None) == 0
    torch.cuda.synchronize()
    if theta == 1.0:
        assert torch.equal(y2, z_prev)
    for a, b in [(y, y2), (g, g2), (z, z2), (x, x2)]:
        assert torch.equal(a, b)
    assert (out.fy, out.lin, out.dxy, out.dzz, out.fx) == (fy.value, terms[0], terms[1], terms[2], fx.value)
    assert out.fk_answered == 1 and out.fk == fk
    assert (out.prox_info[0], out.prox_info[1]) == (info[0], info[1])
    # the trial left the record of f(x): a value evaluation at x is answered with it
    before = stats(lib, f._h)
    assert f(x) == fx.value
    assert stats(lib, f._h) == (before[0] + 1, before[1] + 1)


# ------------------------------------------------------------------ 3. a replayed trial commits nothing
def test_replay_commits_nothing(acc, lib):
    """The record sits AT x_prev, so the trial enqueues its compare; then a stage raises a flag.  REPLAY: the counters
    do not move -- neither for a compare that found a difference nor for one that would have answered --, no record is
    left, and a value evaluation at that address evaluates without a compare."""
    m, n = 300, 3000
    f = acc.DOptimalObj(design(m, n))
    good = point(n, 31)
    keep = good.clone()
    v = f(good)                                                 # the record is at `good`
    assert lib.accbpg_dopt_value_recorded(f._h, ptr(good)) == 1
    fv = C.c_double()

    # the contents equal the record (the compare would answer), z_prev makes y negative
    z_bad = keep.clone()
    z_bad[3] = -1.0                                             # y[3] = 0.5 * good[3] - 0.5 < 0
    before = stats(lib, f._h)
    rc, _, _ = c_trial(lib, f._h, good, z_bad, 0.5, 0.5, 1)
    assert rc == REPLAY
    assert stats(lib, f._h) == before
    assert lib.accbpg_dopt_value_recorded(f._h, ptr(good)) == 0
    assert lib.accbpg_dopt_func_grad_begin(f._h, ptr(good), 0, None) == 0       # no record is left: it evaluates
    assert stats(lib, f._h) == before                                           # ... without a compare
    assert lib.accbpg_dopt_func_grad_end(f._h, C.byref(fv)) == 0
    assert fv.value == v
    assert lib.accbpg_dopt_value_recorded(f._h, ptr(good)) == 1                 # (and that evaluation recorded again)

    # the negative entry written in place into the recorded tensor: the compare finds the difference, the x check fails
    good[3] = -1e-3
    z_prev = keep.clone()
    z_prev[3] = 1e-6                                            # y[3] = 0.5 * (-1e-3) + 0.5 * 1e-6 < 0
    before = stats(lib, f._h)
    rc, _, _ = c_trial(lib, f._h, good, z_prev, 0.5, 0.5, 1)
    assert rc == REPLAY
    assert stats(lib, f._h) == before
    assert lib.accbpg_dopt_value_recorded(f._h, ptr(good)) == 0
    good.copy_(keep)
    torch.cuda.synchronize()
    assert lib.accbpg_dopt_func_grad_begin(f._h, ptr(good), 0, None) == 0
    assert stats(lib, f._h) == before
    assert lib.accbpg_dopt_func_grad_end(f._h, C.byref(fv)) == 0
    assert fv.value == v

    rc, _, _ = c_trial(lib, f._h, good, good, 0.5, 0.0, 1)      # L <= 0: the stepwise prox raises it; REPLAY like any other
    assert rc == REPLAY
    assert stats(lib, f._h) == before
    assert lib.accbpg_dopt_value_recorded(f._h, ptr(good)) == 0


def test_rank_deficient_start_raises_as_the_stepwise_loop(acc):
    shape, iters = SHAPES[0]
    m, n = shape
    x0 = np.zeros(n)
    x0[: m // 2] = 1.0 / (m // 2)                               # support smaller than m: the Gram matrix is singular
    messages = []
    objs = []
    for one_wait in (False, True):
        f = acc.DOptimalObj(design(m, n)).one_wait_trials(one_wait)
        with pytest.raises(ValueError) as err:
            acc.ABPG_gain(f, acc.BurgEntropySimplex(), 1.0, x0, gamma=2, maxitrs=3, verbose=False)
        messages.append(str(err.value))
        objs.append(f)
    assert messages[0] == messages[1] == "HXHT is singular or not positive definite"
    assert objs[1].one_wait_trials_run == 1 and objs[0].calls == objs[1].calls
    # the same objective then solves as if nothing had happened
    want = solve(acc, shape, iters, "overlap", False)
    got = solve(acc, shape, iters, "overlap", True, f=objs[1])
    same_traces(want[0], got[0])
    assert want[1] == got[1] and got[2] == iters - 1


# ------------------------------------------------------------------ 4. the F[k] lookup inside the trial
def test_lookup_guards_inside_the_trial(acc, lib):
    m, n = 300, 3000
    V = design(m, n)
    f, f2 = acc.DOptimalObj(V), acc.DOptimalObj(V)
    a, z_prev = point(n, 41), point(n, 42)
    va = f(a)
    b = a.clone()                                               # the record is at another address: not even a compare
    before = stats(lib, f._h)
    rc, first, out = c_trial(lib, f._h, b, z_prev, 0.4, 0.3, 1)
    assert rc == 0 and out.fk_answered == 0
    assert stats(lib, f._h) == before
    x1 = first[3]                                               # the record is now f(x1) at x1
    rc, asked, out_a = c_trial(lib, f._h, x1, z_prev, 0.4, 0.3, 1)
    assert rc == 0 and out_a.fk_answered == 1 and out_a.fk == out.fx == f2(x1)
    assert stats(lib, f._h) == (before[0] + 1, before[1] + 1)
    rc, plain, out_p = c_trial(lib, f2._h, x1, z_prev, 0.4, 0.3, 0)        # the same trial without the question
    assert rc == 0 and out_p.fk_answered == 0
    for u, v in zip(asked, plain):
        assert torch.equal(u, v)
    assert (out_a.fy, out_a.lin, out_a.dxy, out_a.dzz, out_a.fx) == (out_p.fy, out_p.lin, out_p.dxy, out_p.dzz, out_p.fx)
    # same address, the last entry one ulp further: compared, not answered; the trial's results are those of the
    # stepwise value path
    x2 = asked[3]
    x2[n - 1] = torch.nextafter(x2[n - 1], x2[n - 1] + 1.0)
    before = stats(lib, f._h)
    rc, moved, out_m = c_trial(lib, f._h, x2, z_prev, 0.4, 0.3, 1)
    assert rc == 0 and out_m.fk_answered == 0
    assert stats(lib, f._h) == (before[0] + 1, before[1])
    rc, plain, out_p = c_trial(lib, f2._h, x2, z_prev, 0.4, 0.3, 0)
    assert rc == 0
    for u, v in zip(moved, plain):
        assert torch.equal(u, v)
    assert out_m.fx == out_p.fx and out_m.fy == out_p.fy
    assert va == f2(a)


# ------------------------------------------------------------------ 5. interplay with the other switches
def test_reuse_off_with_one_wait_trials(acc):
    shape, iters = SHAPES[0]
    want = solve(acc, shape, iters, "overlap", False)
    got = solve(acc, shape, iters, "overlap", True, reuse=False)
    same_traces(want[0], got[0])
    assert want[1] == got[1]
    assert got[2] == 0 and got[3] == got[1]["grad"]


@pytest.mark.parametrize("switch", ["linear_gram", "memoize_values", "speculate"])
def test_other_modes_take_the_stepwise_loop(acc, switch):
    V = design(300, 3000)
    f = acc.DOptimalObj(V)
    getattr(f, switch)(True)
    x0 = (1.0 / 3000) * np.ones(3000)
    acc.ABPG_gain(f, acc.BurgEntropySimplex(), 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    assert f.one_wait_trials_run == 0
    getattr(f, switch)(False)
    acc.ABPG_gain(f, acc.BurgEntropySimplex(), 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    assert f.one_wait_trials_run >= 5


def test_a_wrapped_func_grad_is_still_called(acc):
    """An objective whose func_grad was wrapped on the instance is evaluated through the wrapper: the stepwise loop."""
    f = acc.DOptimalObj(design(300, 3000))
    seen = []
    inner = f.func_grad
    f.func_grad = lambda x, flag=2: (seen.append(flag), inner(x, flag))[1]
    x0 = (1.0 / 3000) * np.ones(3000)
    try:
        got = acc.ABPG_gain(f, acc.BurgEntropySimplex(), 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    finally:
        del f.func_grad
    assert f.one_wait_trials_run == 0 and seen.count(2) == f.calls["grad"] >= 5
    want = acc.ABPG_gain(f, acc.BurgEntropySimplex(), 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    assert f.one_wait_trials_run >= 5
    same_traces(want, got)


def test_an_overridden_kernel_method_is_still_called(acc):
    """A BurgEntropySimplex subclass, or one with a method wrapped on the instance, is called through that method."""
    V = design(300, 3000)
    x0 = (1.0 / 3000) * np.ones(3000)
    want = solve(acc, (300, 3000), 5, "overlap", True)

    class Counting(acc.BurgEntropySimplex):
        seen = 0

        def div_prox_map(self, y, g, L):
            Counting.seen += 1
            return super().div_prox_map(y, g, L)

    f = acc.DOptimalObj(V)
    got = acc.ABPG_gain(f, Counting(), 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    assert f.one_wait_trials_run == 0 and Counting.seen == f.calls["grad"] >= 5
    same_traces(want[0], got)

    h = acc.BurgEntropySimplex()
    seen = []
    inner = h.div_prox_map
    h.div_prox_map = lambda y, g, L: (seen.append(L), inner(y, g, L))[1]
    f = acc.DOptimalObj(V)
    got = acc.ABPG_gain(f, h, 1.0, x0, gamma=2, maxitrs=5, verbose=False)
    assert f.one_wait_trials_run == 0 and len(seen) == f.calls["grad"] >= 5
    same_traces(want[0], got)


# ------------------------------------------------------------------ 6. the solver's branches behind an unclean first trial
def _stepped(acc, one_wait, iters, after, poke):
    """ABPG_gain from the uniform start at (300, 3000), `poke(generator locals)` applied after iteration `after`."""
    from accbpg_and_fw_amd.algorithms import ABPG_gain_steps
    V = design(300, 3000)
    f = acc.DOptimalObj(V).one_wait_trials(one_wait)
    x0 = (1.0 / 3000) * np.ones(3000)
    gen = ABPG_gain_steps(f, acc.BurgEntropySimplex(), 1.0, x0, 2, iters, verbose=False)
    out = None
    try:
        while True:
            k = next(gen)
            if k == after:
                poke(gen.gi_frame.f_locals)
                torch.cuda.synchronize()
    except StopIteration as stop:
        out = stop.value
    return f, out


def test_asked_but_not_answered_in_the_solver(acc):
    """x changes in place by one ulp in its last entry between two iterations (same address, under its record): with
    one-wait trials the first trial of the next iteration asks, is not answered, and F[k] is evaluated; the stepwise
    loop compares, finds the difference and evaluates too.  Same traces, same counts."""
    def poke(loc):
        x = loc["x"]
        x[-1] = torch.nextafter(x[-1], x[-1] + 1.0)

    iters, after = 12, 5
    f_off, off = _stepped(acc, False, iters, after, poke)
    f_on, on = _stepped(acc, True, iters, after, poke)
    same_traces(off, on)
    assert len(on[1]) == iters
    assert f_off.calls == f_on.calls
    assert f_on.one_wait_trials_run == f_on.calls["grad"]       # no replay
    assert f_off.values_reused == f_on.values_reused == iters - 2   # F[0] and F[after + 1] were evaluated


def test_replay_in_an_iteration_whose_value_rode_in_the_trial(acc):
    """z gets a negative entry in place between two iterations: the first trial of the next one (which carried the
    F[k] compare) is replayed, and the stepwise calls raise what the stepwise loop raises, from the same call."""
    def poke(loc):
        loc["z"][7] = -0.25                                     # y = (1-theta) x + theta z goes negative there

    seen = []
    for one_wait in (False, True):
        with pytest.raises(AssertionError) as err:
            from accbpg_and_fw_amd.algorithms import ABPG_gain_steps
            V = design(300, 3000)
            f = acc.DOptimalObj(V).one_wait_trials(one_wait)
            gen = ABPG_gain_steps(f, acc.BurgEntropySimplex(), 1.0, (1.0 / 3000) * np.ones(3000), 2, 12, verbose=False)
            seen.append(f)
            while True:
                if next(gen) == 5:
                    poke(gen.gi_frame.f_locals)
                    torch.cuda.synchronize()
        seen.append(str(err.value))
    f_off, msg_off, f_on, msg_on = seen
    assert msg_off == msg_on == "DOptimalObj: x needs to be nonnegative"
    assert f_off.calls == f_on.calls
    assert f_on.one_wait_trials_run == f_on.calls["grad"] + 1   # the last trial was replayed
    # the replay dropped the record: F[6] was started as a full evaluation, not answered (documented difference)
    assert f_on.values_reused == f_off.values_reused - 1 == 5
