"""Guard bands round accbpg_dopt_batch_fw_div_run: the caller's host arrays (prm, active, steps, nrun) carved out of a
sentinel arena (tests/guard_arena.py, on the host side here) -- the call may write the first nsteps records of the active
instances' rows and their nrun entries, nothing else, and reads no entry of an inactive instance -- and a whole solve of
both batch-device solvers with every buffer of the library between two bands (accbpg_debug_guard_bands), bit-identical to
the unbanded solve."""
import ctypes as C

import numpy as np
import pytest

from conftest import gaussian_design
from guard_arena import Arena, View
from test_gpu_guard_internal import env, run_both  # noqa: F401  (env is a fixture)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FILL = 1e-15


@pytest.mark.parametrize("mode", [0, 2], ids=["linesearch", "classical"])
def test_callers_host_arrays(mode):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib as L
    K, m, n, nsteps = 4, 16, 257, 5
    active = [True, False, True, True]
    batch = acc.DOptimalBatch([gaussian_design(m, n, 40 + i) for i in range(K)])
    X, _ = batch.fw_rows(np.ones(n) / n)
    ld = batch.fw_init(X)
    if mode == 2:
        batch.fw_div_probe(None, 1)
    step_doubles = C.sizeof(L.FwDivStep) // 8
    assert C.sizeof(L.FwDivStep) % 8 == 0 and C.sizeof(L.FwDivParams) == 72
    arena = Arena(device="cpu")
    prm_v = arena.carve(9 * K, data=np.zeros(9 * K), name="prm")
    act_v = arena.carve((K + 1) // 2, data=np.zeros((K + 1) // 2), name="active")
    steps_v = arena.carve(K * L.FW_RUN_MAX * step_doubles, name="steps")
    nrun_v = arena.carve((K + 1) // 2, name="nrun")
    arena.snapshot()                                            # (sized by its carves: the views have addresses now)
    prm = (L.FwDivParams * K).from_address(prm_v.ptr)
    act = (C.c_int * K).from_address(act_v.ptr)
    for i in range(K):
        act[i] = 1 if active[i] else 0
        if active[i]:
            prm[i] = L.FwDivParams(mode, 0, 1 + i, 1.0, 2.0, 2.0, 1e-14, ld[i], 0.0, 1e300)
        else:                                                   # (never read: the arena's own pattern would do as well)
            prm[i] = L.FwDivParams(7, 0, -5, float("nan"), 0.0, 0.0, 0.0, float("nan"), 0.0, 0.0)
    arena.snapshot()
    with torch.cuda.device(batch.device):
        rc = batch._lib.accbpg_dopt_batch_fw_div_run(batch._h, FILL, 1.0, prm, nsteps, act,
                                                     C.cast(steps_v.ptr, C.POINTER(L.FwDivStep)),
                                                     C.cast(nrun_v.ptr, C.POINTER(C.c_int)))
    assert rc == L.OK, L.last_error()
    row = L.FW_RUN_MAX * step_doubles
    written = [View("steps[%d][:%d]" % (i, nsteps), steps_v.off + i * row, 1, nsteps * step_doubles,
                    nsteps * step_doubles, steps_v.band, None) for i in range(K) if active[i]]
    # nrun is an int array: its doubles hold two entries each, an inactive one beside an active one among them
    nrun_before = np.frombuffer(arena.snap[nrun_v.off:nrun_v.off + nrun_v.span].numpy().tobytes(), dtype=np.int32)
    arena.check(writable=written + [nrun_v])
    nrun = (C.c_int * K).from_address(nrun_v.ptr)
    for i in range(K):
        if active[i]:
            assert nrun[i] == nsteps, (i, nrun[i])
            recs = (L.FwDivStep * nsteps).from_address(steps_v.ptr + i * row * 8)
            assert all(r.status == L.FW_DIV_APPLIED for r in recs), i
        else:
            assert nrun[i] == nrun_before[i], i


def test_whole_solves_under_library_guard_bands(env):
    acc = env[0]
    m, n, K = 16, 1100, 3

    def scenario():
        batch = acc.DOptimalBatch([gaussian_design(m, n, 60 + i) for i in range(K)])
        x0 = np.ones(n) / n
        out = []
        for replay in ("c", "python"):
            div = acc.D_opt_FW_div_step_batch_device(batch, [1.0, 1e-9, 1.0], x0, 30, 2.0, sync_every=7, refresh=10,
                                                     replay=replay)
            desc = acc.D_opt_FW_descent_step_batch_device(batch, x0, 30, sync_every=7, refresh=10, replay=replay)
            for i in range(K):
                out += [("div %s x %d" % (replay, i), div[i][0]), ("div %s F %d" % (replay, i), div[i][1]),
                        ("div %s Ls %d" % (replay, i), div[i][2]), ("descent %s x %d" % (replay, i), desc[i][0]),
                        ("descent %s F %d" % (replay, i), desc[i][1])]
                out += [("state %s %d %s" % (replay, i, name), t.cpu().numpy())
                        for name, t in zip("xwH", batch.fw_state(i))]
        return out, batch
    run_both(env, scenario, m, 8)
