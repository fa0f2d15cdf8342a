"""The library answers a value evaluation f(x) at the device address and 64-bit content of its last value-only
evaluation from that evaluation's record (include/accbpg_hip.h, accbpg_dopt_value_reuse): the solvers' results must not
change by a bit, every guard of the lookup must hold, and the modes whose values the suite compares must still be
computed when reuse is off."""
import ctypes as C
import math
import time

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


class Counter:
    """Deltas of (compares, answered) on one handle from one call to the next."""

    def __init__(self, lib, h):
        self.lib, self.h = lib, h
        self.last = stats(lib, h)

    def delta(self):
        now = stats(self.lib, self.h)
        d = (now[0] - self.last[0], now[1] - self.last[1])
        self.last = now
        return d


# ------------------------------------------------------------------ 1. traces
def _run(acc, solver, V, iters, reuse, mode):
    f = acc.DOptimalObj(V)
    f.reuse_values(reuse)
    if mode == "serial":
        f.overlap_values(False)
    elif mode == "profile":
        f.profile(True)
    h = acc.BurgEntropySimplex()
    x0 = (1.0 / V.shape[1]) * np.ones(V.shape[1])
    before = f.values_reused
    if solver == "abpg_gain":
        out = acc.ABPG_gain(f, h, 1.0, x0, gamma=2, maxitrs=iters, verbose=False)
    elif solver == "abpg":
        out = acc.ABPG(f, h, 1.0, x0, gamma=2.0, maxitrs=iters, verbose=False)
    else:
        out = acc.BPG(f, h, 1.0, x0, maxitrs=iters, linesearch=True, verbose=False)
    return out, dict(f.calls), f.values_reused - before


@pytest.mark.parametrize("mode", ["overlap", "serial", "profile"])
@pytest.mark.parametrize("shape,iters", [((300, 3000), 60), ((1536, 4096), 30)])
def test_abpg_gain_traces_do_not_change(acc, shape, iters, mode):
    """Every array ABPG_gain returns except the wall-clock stamps T, and the oracle-call counts, are the same with
    reuse off and on; with it on every F[k], k >= 1, is answered (the accepting test evaluated that very x) and nothing
    else is.  Small tile with the one-launch Cholesky, and big tile with the side handle in small launches; F[k] on the
    side stream, on the solver's stream, and with kernel timing on (the benchmark's timed region)."""
    V = design(*shape)
    off, calls_off, reused_off = _run(acc, "abpg_gain", V, iters, False, mode)
    on, calls_on, reused_on = _run(acc, "abpg_gain", V, iters, True, mode)
    assert len(off) == len(on) == 6
    assert len(on[1]) == iters                                  # (no early stop: the count below means something)
    for a, b in zip(off[:-1], on[:-1]):
        np.testing.assert_array_equal(a, b)
    assert calls_off == calls_on
    assert reused_off == 0
    assert reused_on == len(on[1]) - 1


@pytest.mark.parametrize("solver", ["abpg", "bpg"])
def test_solvers_without_a_repeat_are_untouched(acc, solver):
    """ABPG and BPG with line search never ask for a value twice: same traces, nothing answered."""
    V = design(300, 3000)
    off, calls_off, reused_off = _run(acc, solver, V, 40, False, "overlap")
    on, calls_on, reused_on = _run(acc, solver, V, 40, True, "overlap")
    for a, b in zip(off[:-1], on[:-1]):
        np.testing.assert_array_equal(a, b)
    assert calls_off == calls_on
    assert reused_off == 0 and reused_on == 0


# ------------------------------------------------------------------ 2. guards
@pytest.mark.parametrize("n", [3000, 3001, 129 + 300])
def test_lookup_guards(acc, lib, n):
    m = 300
    V = design(m, n)
    f = acc.DOptimalObj(V)
    cnt = Counter(lib, f._h)
    x = point(n, 7 + n)

    v = f(x)
    assert cnt.delta() == (0, 0)                                # nothing recorded yet: no compare
    assert f(x) == v
    assert cnt.delta() == (1, 1)                                # the same tensor: answered, the same bits

    x.mul_(1.5)                                                 # same address, every entry different
    v15 = f(x)
    assert cnt.delta() == (1, 0)
    want = v - m * math.log(1.5)
    assert abs(v15 - want) <= 1e-12 * abs(want)

    for idx in (0, n - 1):                                      # one ulp in the first / the last entry
        assert f(x) == v15
        assert cnt.delta() == (1, 1)
        x[idx] = torch.nextafter(x[idx], x[idx] + 1.0)
        v15 = f(x)
        assert cnt.delta() == (1, 0)

    y = x.clone()                                               # other address: not even a compare
    assert f(y) == v15
    assert cnt.delta() == (0, 0)
    assert f(y) == v15
    assert cnt.delta() == (1, 1)

    # a view that starts one element in (8-byte aligned only), through the C ABI
    buf = torch.zeros(n + 1, dtype=torch.float64, device="cuda")
    buf[1:] = x
    torch.cuda.synchronize()
    fv = C.c_double()
    assert lib.accbpg_dopt_func_grad(f._h, C.c_void_p(buf.data_ptr() + 8), 0, C.byref(fv), None) == 0
    assert cnt.delta() == (0, 0)
    vb = fv.value
    assert abs(vb - v15) <= 1e-11 * abs(v15)                    # (the suite's bound between two routes to the same f)
    assert lib.accbpg_dopt_func_grad(f._h, C.c_void_p(buf.data_ptr() + 8), 0, C.byref(fv), None) == 0
    assert cnt.delta() == (1, 1) and fv.value == vb
    buf[n] = torch.nextafter(buf[n], buf[n] + 1.0)              # its last entry
    torch.cuda.synchronize()
    assert lib.accbpg_dopt_func_grad(f._h, C.c_void_p(buf.data_ptr() + 8), 0, C.byref(fv), None) == 0
    assert cnt.delta() == (1, 0)
    buf[1] = torch.nextafter(buf[1], buf[1] + 1.0)              # its first entry
    torch.cuda.synchronize()
    assert lib.accbpg_dopt_func_grad(f._h, C.c_void_p(buf.data_ptr() + 8), 0, C.byref(fv), None) == 0
    assert cnt.delta() == (1, 0)

    # a gradient evaluation elsewhere neither writes nor clears the record
    v = f(x)
    assert cnt.delta() == (0, 0)
    other = point(n, 99)
    fo, _ = f.func_grad(other, 2)
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)
    assert f(other) == fo                                       # f alone after a gradient there: computed
    assert cnt.delta() == (0, 0)

    # errors drop the record: the next good evaluation is computed, the one after it answered
    bad = x.clone()
    bad[3] = -1e-3
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    with pytest.raises(AssertionError):
        f(bad)
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)
    flat = torch.zeros(n, dtype=torch.float64, device="cuda")
    flat[: m // 2] = 1.0 / (m // 2)                             # rank m/2
    with pytest.raises(ValueError):
        f(flat)
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)

    # a switch of how the factorisation runs drops it too
    assert lib.accbpg_debug_chol_variant(f._h, 0) == 0
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)
    assert lib.accbpg_dopt_factor_in_small_launches(f._h, 0) == 0
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)

    # and the switch itself
    f.reuse_values(False)
    assert f(x) == v and f(x) == v
    assert cnt.delta() == (0, 0)
    f.reuse_values(True)
    assert f(x) == v
    assert cnt.delta() == (0, 0)
    assert f(x) == v
    assert cnt.delta() == (1, 1)


# ------------------------------------------------------------------ 3. modes still compared for real
@pytest.mark.parametrize("shape", [(1536, 4096), (512, 2048)])
def test_factorisation_modes_computed_with_reuse_off(acc, lib, shape):
    """With reuse off every f(x) runs: the launch-per-block-column factorisation (small-launch modes 1 and 2, debug bit
    6) and the one launch give the same value to the bit, each of them computed."""
    m, n = shape
    f = acc.DOptimalObj(design(m, n)).reuse_values(False)
    x = point(n, 5)
    want = f(x)
    for call, arg in [(lib.accbpg_dopt_factor_in_small_launches, 1), (lib.accbpg_dopt_factor_in_small_launches, 2),
                      (lib.accbpg_dopt_factor_in_small_launches, 0), (lib.accbpg_debug_chol_variant, 64),
                      (lib.accbpg_debug_chol_variant, 0)]:
        assert call(f._h, arg) == 0
        assert f(x) == want
    assert stats(lib, f._h) == (0, 0)
    assert f.values_reused == 0


# ------------------------------------------------------------------ 4. redo
def test_redo_of_an_abandoned_factorisation_evaluates_and_records(acc, lib):
    """The one-launch Cholesky gives up its wait (test hook, bounded spin): the redo inside _end evaluates -- it never
    looks up -- and leaves a record the next f(x) is answered from."""
    V = design(512, 2048)
    x = point(2048, 3)
    want = acc.DOptimalObj(V)(x)
    g = acc.DOptimalObj(V)
    assert lib.accbpg_debug_chol_variant(g._h, 128) == 0         # bit 7: stall + 2 ms spin limit
    cnt = Counter(lib, g._h)
    t0 = time.time()
    got = g(x)
    assert time.time() - t0 < 5.0
    assert got == want
    assert cnt.delta() == (0, 0)
    assert g(x) == want
    assert cnt.delta() == (1, 1)


# ------------------------------------------------------------------ 5. begin / end
def test_begin_end_answered_through_the_c_abi(acc, lib):
    n = 3000
    f = acc.DOptimalObj(design(300, n))
    h, h2 = f._h, f._side_handle()
    x, y = point(n, 11), point(n, 12)
    v = f(x)
    fy, gy = f.func_grad(y, 2)
    torch.cuda.synchronize()
    fv = C.c_double()

    c1 = Counter(lib, h)
    assert lib.accbpg_dopt_func_grad_begin(h, C.c_void_p(x.data_ptr()), 0, None) == 0
    assert c1.delta() == (1, 1)
    assert lib.accbpg_dopt_func_grad_end(h, C.byref(fv)) == 0
    assert fv.value == v

    c2 = Counter(lib, h2)                                       # the side handle answers from its peer's record
    assert lib.accbpg_dopt_func_grad_begin(h2, C.c_void_p(x.data_ptr()), 0, None) == 0
    assert c2.delta() == (1, 1)
    fv.value = 0.0
    assert lib.accbpg_dopt_func_grad_end(h2, C.byref(fv)) == 0
    assert fv.value == v
    ms = C.c_double()
    assert lib.accbpg_dopt_eval_gap_ms(h2, h, C.byref(ms)) == 0
    assert lib.accbpg_dopt_eval_gap_ms(h, h2, C.byref(ms)) == 0

    dropped = f.grad_async(y)                                   # in flight on the side stream, never waited for
    f.grad_drop(dropped)
    assert f.value_wait(f.value_async(x)) == v
    assert c2.delta() == (1, 1)
    assert f.value_lead_seconds() >= 0.0
    f2, g2 = f.grad_wait(f.grad_async(y))                       # a fresh one is its own evaluation
    assert f2 == fy
    assert torch.equal(g2, gy)
    assert f.value_wait(f.value_async(x)) == v                  # and the record is still there
    assert c2.delta() == (1, 1)
