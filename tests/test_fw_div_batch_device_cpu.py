"""The host side of D_opt_FW_div_step_batch_device / D_opt_FW_descent_step_batch_device without a GPU: the public names
and the two C-ABI entries, where the chunks of a batch are cut, which instances every call covers, the replay of each
instance's records in C and in Python, the roll-back of ONE instance on a disagreement, the hand-backs and the drift of
the instances' iteration numbers.  tests/fwdiv_batch_fake.FakeBatch stands in for the device (one fwdiv_numpy.State per
instance, its own predictor of the device's decisions); every instance must come out bit for bit as fwdiv_numpy's solver
run on it alone.  The C replay goes through ctypes: accbpg_fw_div_replay is a pure host function and the library loads
without a GPU (as in test_abi_cpu.py)."""
import inspect
import os
import re

import numpy as np
import pytest

import fwdiv_batch_fake as FB
import fwdiv_numpy as R
from conftest import gaussian_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["accbpg_dopt_batch_fw_div_run", "accbpg_fw_div_replay"]
M, N, ITERS = 30, 1000, 150
REPLAYS = ("c", "python")


def _alg():
    from accbpg_and_fw_amd import D_opt_alg
    return D_opt_alg


_designs = {}


def designs(K):
    for i in range(K):
        if i not in _designs:
            _designs[i] = gaussian_design(M, N, 12 + i)
    return [_designs[i] for i in range(K)], np.ones(N) / N


_refs = {}


def ref_div(i, L=1.0, iters=ITERS, **kw):
    """fwdiv_numpy's solver on instance i alone: once per argument set, left unchanged."""
    key = ("div", i, L, iters, tuple(sorted(kw.items())))
    if key not in _refs:
        Vs, x0 = designs(i + 1)
        _refs[key] = R.fw_div_step(Vs[i], L, x0, iters, 2.0, **kw)
    return _refs[key]


def ref_descent(i, iters=ITERS, **kw):
    key = ("descent", i, iters, tuple(sorted(kw.items())))
    if key not in _refs:
        Vs, x0 = designs(i + 1)
        _refs[key] = R.fw_descent_step(Vs[i], x0, iters, **kw)
    return _refs[key]


def same(got, want, what):
    assert len(got[1]) == len(want[1]), (what, len(got[1]), len(want[1]))
    for a, b in zip(got, want):                                 # (want is shorter: x, F[, Ls])
        np.testing.assert_array_equal(a, b, err_msg=str(what))


def run_div(K, L=1.0, iters=ITERS, S=64, replay="c", prepare=None, **kw):
    Vs, x0 = designs(K)
    batch, stats = FB.FakeBatch(Vs), {}
    if prepare:
        prepare(batch)
    out = _alg().D_opt_FW_div_step_batch_device(batch, L, x0, iters, 2.0, sync_every=S, stats=stats, replay=replay, **kw)
    return out, stats, batch


def run_descent(K, iters=ITERS, S=64, replay="c", prepare=None, **kw):
    Vs, x0 = designs(K)
    batch, stats = FB.FakeBatch(Vs), {}
    if prepare:
        prepare(batch)
    out = _alg().D_opt_FW_descent_step_batch_device(batch, x0, iters, sync_every=S, stats=stats, replay=replay, **kw)
    return out, stats, batch


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_names_signatures_and_entries():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    D = _alg()
    E = inspect.Parameter.empty
    Rf, Sy = D.REFRESH_DEFAULT, D.SYNC_EVERY_DEFAULT
    div = [("batch", E), ("L", E), ("x0", E), ("maxitrs", E), ("gamma", E), ("epsilon", 1e-14), ("linesearch", True),
           ("ls_ratio", 2), ("radius", 1), ("refresh", Rf), ("sync_every", Sy), ("stats", None), ("replay", "c")]
    desc = [("batch", E), ("x0", E), ("maxitrs", E), ("epsilon", 1e-14), ("radius", 1), ("refresh", Rf),
            ("sync_every", Sy), ("stats", None), ("replay", "c")]
    for name in ("D_opt_FW_div_step_batch_device", "D_opt_FW_descent_step_batch_device"):
        assert name in acc.__all__ and callable(getattr(acc, name))
    assert _sig(acc.D_opt_FW_div_step_batch_device) == _sig(D.D_opt_FW_div_step_batch_device_steps) == div
    assert _sig(acc.D_opt_FW_descent_step_batch_device) == _sig(D.D_opt_FW_descent_step_batch_device_steps) == desc
    assert inspect.isgeneratorfunction(D.D_opt_FW_div_step_batch_device_steps)
    assert inspect.isgeneratorfunction(D.D_opt_FW_descent_step_batch_device_steps)
    for name in ("fw_div_run", "fw_snapshot", "fw_restore", "fw_div_replay"):
        assert callable(getattr(acc.DOptimalBatch, name))
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.accbpg_abi_version() == 3


def test_decisions_are_shared():
    """The batch-device generators write no decision of their own: the per-record code is the single-handle device
    solvers', over the sequential solvers' _DivStepRun / _DescentRun."""
    D = _alg()
    for fn in (D.D_opt_FW_div_step_batch_device_steps, D.D_opt_FW_descent_step_batch_device_steps, D._div_replay_chunk,
               D._descent_replay_chunk):
        src = inspect.getsource(fn)
        assert "_step_length" not in src and "_SLOPE_FLOOR" not in src and "ls_ratio *" not in src
        assert "sum_w2" not in src and "2 / (k + 2)" not in src and "_same_bits" not in src
    assert "_div_replay_records(" in inspect.getsource(D._div_replay_chunk)
    assert "_div_replay_records(" in inspect.getsource(D._div_device_steps)
    assert "_descent_replay_records(" in inspect.getsource(D._descent_replay_chunk)
    assert "_descent_replay_records(" in inspect.getsource(D._descent_device_steps)


@pytest.mark.parametrize("refresh", [0, 1, 5, 256])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_whole_runs_and_chunk_cuts(refresh, S):
    K = 3
    for replay in REPLAYS:
        out, stats, batch = run_div(K, S=S, replay=replay, refresh=refresh)
        for i in range(K):
            same(out[i][:3], ref_div(i, refresh=refresh), ("div", refresh, S, replay, i))
            assert len(out[i][3]) == len(out[i][1])
        assert stats["rollbacks"] == 0 and stats["handed_back"] == 0
        runs = [c for c in batch.log if c[0] == "run"]
        assert stats["chunks"] == sum(len(c[1]) for c in runs)
        for _, idx, nsteps, k0s in runs:                        # no chunk spans a refresh; all instances run together
            assert idx == (0, 1, 2) and len(set(k0s)) == 1 and 1 <= nsteps <= S
            assert not refresh or k0s[0] % refresh + nsteps <= refresh
        if S == 64 and refresh in (0, 256):
            assert [(c[3][0], c[2]) for c in runs] == [(0, 64), (64, 64), (128, 22)]
        out, stats, batch = run_descent(K, S=S, replay=replay, refresh=refresh)
        for i in range(K):
            same(out[i][:2], ref_descent(i, refresh=refresh), ("descent", refresh, S, replay, i))
            assert len(out[i][2]) == len(out[i][3]) == len(out[i][1]) and not out[i][3].any()
        assert stats["rollbacks"] == 0 and stats["handed_back"] == 0
        runs = [c for c in batch.log if c[0] == "run"]
        for _, idx, nsteps, k0s in runs:                        # ... nor ends on the step that makes one due
            assert 1 <= nsteps <= S and (not refresh or (k0s[0] - 1) % refresh + nsteps < refresh)
        if refresh == 1:
            assert runs == []
        if refresh == 5:
            assert batch.inits == [1 + (ITERS - 1) // 5] * K


def _stop_epsilon(F, kstop):
    d = np.abs(np.diff(F))
    lo = d[:kstop - 1].min() if kstop > 1 else np.inf
    return None if not d[kstop - 1] < lo else float((d[kstop - 1] + min(lo, 2 * d[kstop - 1] + 1.0)) / 2)


def test_staggered_stops_and_the_active_set_of_every_call():
    """K = 5 instances, per-instance L: they stop at different iterations (the epsilon is taken from instance 0's own F
    so that it stops in mid-chunk), and every call covers exactly the instances still running."""
    K, Ls = 5, [1.0, 2.0, 0.5, 4.0, 1.5]
    F0 = ref_div(0, Ls[0])[1]
    kstop, eps = next((k, _stop_epsilon(F0, k)) for k in range(24, 140, 7) if _stop_epsilon(F0, k) is not None)
    want = [ref_div(i, Ls[i], epsilon=eps) for i in range(K)]
    lengths = [len(w[1]) for w in want]
    print("epsilon %.3e, lengths %r" % (eps, lengths))
    assert lengths[0] == kstop + 1 and len(set(lengths)) >= 3 and kstop % 7 == 3
    results = []
    for replay in REPLAYS:
        out, stats, batch = run_div(K, L=Ls, S=7, replay=replay, epsilon=eps)
        for i in range(K):
            same(out[i][:3], want[i], ("stops", replay, i))
        for call in batch.log:
            if call[0] == "run":                                # the chunk that starts at k covers those with more to do
                k0 = call[3][0]
                assert set(call[3]) == {k0} and call[1] == tuple(i for i in range(K) if lengths[i] > k0), call
            if call[0] == "snapshot":
                assert call[1] == next(c[1] for c in batch.log[batch.log.index(call):] if c[0] == "run")
        assert stats["rollbacks"] == 0 and batch.restored == []
        results.append((stats, [c for c in batch.log if c[0] == "run"]))
    assert results[0] == results[1]
    wantd = [ref_descent(i, epsilon=1e-3) for i in range(K)]
    for replay in REPLAYS:
        out, stats, batch = run_descent(K, S=7, replay=replay, epsilon=1e-3)
        for i in range(K):
            same(out[i][:2], wantd[i], ("descent stops", replay, i))
        for call in batch.log:
            if call[0] == "run":
                assert call[1] == tuple(i for i in range(K) if len(wantd[i][1]) > call[3][0]), call


@pytest.mark.parametrize("kind", ["accept", "ulp", "stop"])
def test_planted_disagreement_restores_one_instance(kind):
    """Falsified predictions on instance 1 alone (first, middle and last record of a chunk of 7, two in a row) and one
    on instance 2: only those instances are restored, the count is exact, and the instances run on at different k."""
    K = 3
    planted = {(1, 7): kind, (1, 10): kind, (1, 13): kind, (1, 14): kind, (2, 40): kind}
    results = []
    for replay in REPLAYS:
        out, stats, batch = run_div(K, S=7, replay=replay, prepare=lambda b: b.flips.update(planted))
        for i in range(K):
            same(out[i][:3], ref_div(i), ("planted", kind, replay, i))
        assert stats["rollbacks"] == len(planted) and batch.flips == {}
        assert batch.restored.count(1) == 4 and batch.restored.count(2) == 1 and 0 not in batch.restored
        drift = [dict(zip(c[1], c[3])) for c in batch.log if c[0] == "run" and len(set(c[3])) > 1]
        assert drift, "the instances never ran at different iteration numbers"
        assert all(k0s[0] > k0s[1] for k0s in drift if 0 in k0s and 1 in k0s)     # instance 1 fell behind instance 0
        results.append((stats, batch.restored, [c for c in batch.log if c[0] == "run"]))
    assert results[0] == results[1]
    if kind == "accept":
        return
    planted = {(1, 8): kind, (1, 10): kind, (1, 14): kind, (1, 15): kind, (2, 40): kind}
    results = []
    for replay in REPLAYS:
        out, stats, batch = run_descent(K, S=7, replay=replay, prepare=lambda b: b.flips.update(planted))
        for i in range(K):
            same(out[i][:2], ref_descent(i), ("planted descent", kind, replay, i))
        assert stats["rollbacks"] == len(planted) and batch.flips == {}
        assert batch.restored.count(1) == 4 and batch.restored.count(2) == 1 and 0 not in batch.restored
        results.append((stats, batch.restored, [c for c in batch.log if c[0] == "run"]))
    assert results[0] == results[1]


def test_capped_step_on_one_instance_and_the_next_chunk_length():
    """Instance 1 starts from a tiny L: its first iteration sits at the cap, is handed back and re-initialises that
    instance alone (its ``since`` is reset); the other instances keep their chunk.  With refresh = 10 the next chunk is
    as long as the shortest of the per-instance limits."""
    K, Ls = 3, [1.0, 1e-9, 1.0]
    for linesearch in (True, False):
        results = []
        for replay in REPLAYS:
            out, stats, batch = run_div(K, L=Ls, iters=40, S=7, replay=replay, refresh=10, linesearch=linesearch)
            for i in range(K):
                same(out[i][:3], ref_div(i, Ls[i], 40, refresh=10, linesearch=linesearch), ("cap", linesearch, replay, i))
            print("linesearch", linesearch, replay, stats, "inits", batch.inits)
            assert stats["handed_back"] >= 1 and stats["rollbacks"] == 0 and batch.restored == []
            runs = [c for c in batch.log if c[0] == "run"]
            assert runs[0][2] == 7 and runs[0][3] == (0, 0, 0)
            if not linesearch:                                  # the capped step was taken: instance 1 is one iteration
                assert runs[1][3] == (7, 1, 7)                  # on, its since is 0; the others have 3 steps to the refresh
                assert runs[1][2] == 3 and batch.inits[1] > batch.inits[0]
            results.append((stats, runs))
        assert results[0] == results[1]


@pytest.mark.parametrize("reason,fields,exc,msg", [
    (FB.SLOPE, dict(slope=2e-6), ValueError, "instance 1: grad_d_prod must be non-positive"),
    (FB.MIN_X, dict(min_x=0.0), AssertionError, "instance 1: Entries of x or y not positive."),
    (FB.PIVOT, dict(i=N), ValueError, "instance 1: accbpg_fw_div_probe_step: bad argument"),
], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_errors_name_the_instance(reason, fields, exc, msg):
    """What the sequential solver raises is raised with the instance in front, for both replays: the record is planted
    into the probes of instance 1 from its 9th step on."""
    K = 3

    def prepare(batch):
        real = batch._probe

        def probe(i):
            rec = real(i)
            if i == 1 and batch.steps_applied(1) >= 9:
                batch.recs[1].update(fields)
                for k, v in fields.items():
                    setattr(rec, k, v)
            return rec
        batch._probe = probe
    for replay in REPLAYS:
        with pytest.raises(exc) as got:
            run_div(K, S=7, replay=replay, iters=30, prepare=prepare)
        assert str(got.value).startswith(msg), str(got.value)


def test_arguments():
    D = _alg()
    Vs, x0 = designs(2)
    with pytest.raises(ValueError, match="replay"):
        D.D_opt_FW_div_step_batch_device(FB.FakeBatch(Vs), 1.0, x0, 10, 2.0, replay="both")
    with pytest.raises(ValueError, match="sync_every"):
        D.D_opt_FW_div_step_batch_device(FB.FakeBatch(Vs), 1.0, x0, 10, 2.0, sync_every=0)
    with pytest.raises(ValueError, match="instance 1: Initial L must be positive"):
        D.D_opt_FW_div_step_batch_device(FB.FakeBatch(Vs), [1.0, -1.0], x0, 10, 2.0)
    out = D.D_opt_FW_div_step_batch_device(FB.FakeBatch(Vs), 1.0, x0, 1, 2.0)
    assert [len(r[1]) for r in out] == [1, 1]
    out = D.D_opt_FW_descent_step_batch_device(FB.FakeBatch(Vs), x0, 1)
    assert [len(r[1]) for r in out] == [1, 1]
