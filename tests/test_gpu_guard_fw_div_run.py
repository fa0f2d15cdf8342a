"""Guard bands for the device-decided Bregman-step runs.

The caller's device buffers of accbpg_fw_set_state (x, w, H; read only) and of accbpg_fw_get_state (written whole) are
carved out of one arena filled with a sentinel (tests/guard_arena.py): no double outside the named outputs may change,
and the state restored from the arena has the bits of the state saved into it -- with a run of accbpg_fw_div_run in
between in both modes.  Shapes: m = 13 and 16 (H of 169 and 256 doubles), n odd, at and across the 1024-entry block
of the reductions, x at 16 bytes and at 8 mod 16.

The library's OWN buffers (the run slot, the workspace of the probe, the Frank-Wolfe state) are banded with
accbpg_debug_guard_bands around whole device-decided solves, as tests/test_gpu_guard_internal.py does for the other
paths: no band may be damaged and the results must have the bits of the unbanded run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402
from test_gpu_guard_internal import DOPT_HANDLE_BUFFERS, env, gaussian, run_both  # noqa: E402,F401  (env: a fixture)

pytestmark = pytest.mark.gpu

FILL = 1e-15


def P(v):
    return C.c_void_p(v.ptr)


def ok(rc, what):
    from accbpg_and_fw_amd import _lib
    assert rc == 0, "%s returned %d: %s" % (what, rc, _lib.last_error())


def _run(L, lib, h, mode, k0, nsteps, ld, q, F_prev):
    prm = L.FwDivParams(mode, 0, k0, 1.0, 2.0, 2.0, 1e-14, ld, q, F_prev)
    steps = (L.FwDivStep * nsteps)()
    nrun = C.c_int(0)
    ok(lib.accbpg_fw_div_run(h, FILL, 1.0, C.byref(prm), nsteps, steps, C.byref(nrun)), "fw_div_run")
    assert nrun.value == nsteps
    return steps


def state_case(A, m, n, skew):
    from accbpg_and_fw_amd import _lib as L
    lib = L.load()
    rng = np.random.RandomState(m * 31 + n)
    V = torch.from_numpy(rng.randn(m, n)).cuda()
    x0 = torch.full((n,), 1.0 / n, dtype=torch.float64, device="cuda")
    xs, ws = A.carve(n, skew=skew, name="x_saved"), A.carve(n, name="w_saved")
    Hs = A.carve(m * m, skew=skew, name="H_saved")
    xo, wo, Ho = A.carve(n, name="x_out"), A.carve(n, skew=skew, name="w_out"), A.carve(m * m, name="H_out")
    A.snapshot()
    h = C.c_void_p()
    ok(lib.accbpg_dopt_create(C.c_void_p(V.data_ptr()), m, n, n, None, C.byref(h), 0), "dopt_create")
    res = []
    try:
        ld = C.c_double(0.0)
        ok(lib.accbpg_fw_init(h, C.c_void_p(x0.data_ptr()), C.byref(ld)), "fw_init")
        first = _run(L, lib, h, L.FW_DIV_LINESEARCH, 0, 5, ld.value, 0.0, 0.0)
        ok(lib.accbpg_fw_get_state(h, P(xs), P(ws), P(Hs)), "fw_get_state")
        A.check(writable=[xs, ws, Hs], whole=[xs, ws, Hs])
        A.snapshot()
        book = (first[4].ld1, first[4].q1, 0.0)
        steps = _run(L, lib, h, L.FW_DIV_LINESEARCH, 5, 9, *book)
        rec = L.FwDivProbe()
        ok(lib.accbpg_fw_div_probe_step(h, FILL, 1.0, C.byref(rec)), "fw_div_probe_step")
        _run(L, lib, h, L.FW_DIV_CLASSICAL, 14, 6, steps[8].ld1, steps[8].q1, 0.0)
        ok(lib.accbpg_fw_set_state(h, P(xs), P(ws), P(Hs)), "fw_set_state")
        ok(lib.accbpg_fw_get_state(h, P(xo), P(wo), P(Ho)), "fw_get_state")
        A.check(writable=[xo, wo, Ho], whole=[xo, wo, Ho])      # the saved state was read, not written
        for a, b in ((xs, xo), (ws, wo), (Hs, Ho)):
            assert np.array_equal(A.bits_of(a), A.bits_of(b)), a.name
        again = _run(L, lib, h, L.FW_DIV_LINESEARCH, 5, 9, *book)
        res.append(("records", np.frombuffer(bytes(again), dtype=np.int64).copy()))
        assert bytes(again) == bytes(steps)
        A.check(writable=[xo, wo, Ho])
    finally:
        torch.cuda.synchronize()
        lib.accbpg_dopt_destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in (xs, ws, Hs)]


@pytest.mark.parametrize("m,n,skew", [(13, 506, 0), (16, 1023, 1), (16, 1025, 0), (13, 4097, 1)])
def test_state_buffers_of_the_caller(m, n, skew):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    got = state_case(GA.Arena(), m, n, skew)
    want = state_case(GA.Plain(), m, n, skew)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert np.array_equal(a, b), "%s differs from the run on plain allocations" % name


@pytest.mark.parametrize("m,n", [(13, 506), (64, 1025)])
def test_device_decided_solves_under_bands(env, m, n):
    """fw_x, fw_w, fw_H, fw_hv, the probe's workspace and the run slot on top of the handle's own buffers"""
    acc, lib, _ = env
    V = gaussian(m, n, 17)

    def scenario():
        f = acc.DOptimalObj(V)
        x0 = np.ones(n) / n
        stats = {}
        x, F, Ls, _ = acc.D_opt_FW_div_step_device(f, 1.0, x0, 40, 2.0, verbose=False, sync_every=7, refresh=16,
                                                   stats=stats)
        xd, Fd, _, _ = acc.D_opt_FW_descent_step_device(f, x0, 40, verbose=False, sync_every=7, refresh=16)
        xc, Fc, Lc, _ = acc.D_opt_FW_div_step_device(f, 1e-9, x0, 12, 2.0, verbose=False, sync_every=5)  # hand-backs
        return [("x", x), ("F", F), ("Ls", Ls), ("xd", xd), ("Fd", Fd), ("xc", xc), ("Fc", Fc), ("Lc", Lc)], f

    run_both(env, scenario, m, DOPT_HANDLE_BUFFERS + 6)
