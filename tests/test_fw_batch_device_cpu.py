"""The host side of D_opt_FW_batch_device / D_opt_FW_away_batch_device without a GPU: the replay of every instance's
records of ``accbpg_dopt_batch_fw_run`` through the solvers' one copy of the decisions, the bit-for-bit guard, the active
set between chunks and where the chunks are cut.

``NumpyBatch`` stands in for the batch: one ``NumpyRun`` of tests/test_fw_device_cpu.py per instance (state in NumPy,
the device's decisions restated in Python floats, a stop in mid-chunk, status 2 for a pivot outside [0, n)).  Like the
device it runs the active instances only and returns, per active instance, the records up to the stop."""
import inspect
import os
import re

import numpy as np
import pytest

import fw_numpy as N
from conftest import gaussian_design
from oracle import np_oracle as O
from test_fw_device_cpu import INF, INT64_MAX, NAN, NumpyRun, _drain, run_away, run_fw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _alg():
    from accbpg_and_fw_amd import D_opt_alg
    return D_opt_alg


class NumpyBatch:
    """What the batch-device solvers ask of an initialised batch, in NumPy."""

    def __init__(self, Vs, x0s):
        self.inst = [NumpyRun(V, x0) for V, x0 in zip(Vs, x0s)]
        self.K, self.m = len(self.inst), self.inst[0].m
        self.logdet = [st.logdet_gram for st in self.inst]
        self.calls = []             # (first iteration of the running instances, nsteps, active set) of every fw_run
        self.snaps = []             # (iteration, active set) of every fw_logdet_snapshot
        self.k = 0

    def fw_run(self, away, eps, nsteps, active=None):
        active = [True] * self.K if active is None else list(active)
        assert len(eps) == self.K
        self.calls.append((self.k, nsteps, tuple(active)))
        self.k += nsteps
        return [self.inst[i].run(away, eps[i], nsteps) if active[i] else None for i in range(self.K)]

    def bad_pivot(self):
        raise ValueError("accbpg_fw_update: bad argument (pivot index outside [0, n))")

    def fw_x(self, i, as_numpy=True):
        return self.inst[i].x()

    def fw_logdet_ring(self, depth):
        for st in self.inst:
            st.logdet_ring(depth)

    def fw_logdet_snapshot(self, active=None):
        active = [True] * self.K if active is None else list(active)
        self.snaps.append((self.k, tuple(active)))
        return [self.inst[i].snapshot() if active[i] else NAN for i in range(self.K)]

    def fw_logdet_flush(self, i):
        return self.inst[i].flush_logdet()


def batch_fw(b, eps, maxitrs, S):
    eps = [float(v) for v in np.broadcast_to(eps, (b.K,))]
    return _drain(_alg()._fw_batch_device_steps(b, b.logdet, eps, maxitrs, S, 0.0))


def batch_away(b, eps, maxitrs, S, R=None, ring=None):
    eps = [float(v) for v in np.broadcast_to(eps, (b.K,))]
    return _drain(_alg()._away_batch_device_steps(b, b.logdet, eps, maxitrs, S, R, ring, 0.0))


def _axis_batch(starts=(0, 4, 8), m=8, n=40):
    Vs, x0s = [], []
    for start in starts:
        s, x0 = N.axis_run_design(m, n, start)
        V, G = N.axis_design(m, n, s, x0)
        Vs.append(V)
        x0s.append(x0)
    return Vs, x0s


def _same(got, want, what=""):
    for a, b in zip(got[:4], want[:4]):
        np.testing.assert_array_equal(a, b, err_msg=str(what))
    assert len(got[4]) == len(want[4])


# ------------------------------------------------------------------------------------------ replay against the oracle
@pytest.mark.parametrize("S", [1, 7, 64])
@pytest.mark.parametrize("eps", [-1.0, 1.0])
def test_replay_is_the_oracle_bit_for_bit_on_axis_designs(S, eps):
    """Three (8, 40) axis designs, 60 iterations; eps = 1 stops every instance before the chunks run out.  Every
    instance of the batch equals the oracle where the single replay does (plain: all of it; away with a factorisation
    per iteration: all of it), and the single replay bit for bit throughout."""
    Vs, x0s = _axis_batch()
    K = len(Vs)
    assert not np.array_equal(Vs[0], Vs[1])
    res = batch_fw(NumpyBatch(Vs, x0s), eps, 60, S)
    assert len(res) == K
    for i in range(K):
        want = O.D_opt_FW(Vs[i], x0s[i], eps, 60)
        assert len(want[1]) == len(res[i][1]) and (eps < 0 or 2 < len(res[i][1]) < 60)
        _same(res[i], want, ("FW oracle", i))
        _same(res[i], run_fw(NumpyRun(Vs[i], x0s[i]), eps, 60, S), ("FW single", i))
    for ring in (1, 3):
        res = batch_away(NumpyBatch(Vs, x0s), eps, 60, S, R=1, ring=ring)
        for i in range(K):
            _same(res[i], O.D_opt_FW_away(Vs[i], x0s[i], eps, 60), ("away oracle", i, ring))
    for R in (0, 5, 16, None):
        res = batch_away(NumpyBatch(Vs, x0s), eps, 60, S, R=R)
        for i in range(K):
            _same(res[i], run_away(NumpyRun(Vs[i], x0s[i]), eps, 60, S, R=R), ("away single", i, R))


def test_x0_and_eps_per_instance():
    """eps per instance: instance 1 stops at once, the others run on with theirs"""
    Vs, x0s = _axis_batch()
    b = NumpyBatch(Vs, x0s)
    res = batch_fw(b, [-1.0, 1e30, 1.0], 60, 7)
    assert len(res[0][1]) == 60 and len(res[1][1]) == 1 and 2 < len(res[2][1]) < 60
    np.testing.assert_array_equal(res[1][0], x0s[1])
    for i, eps in enumerate([-1.0, 1e30, 1.0]):
        _same(res[i], O.D_opt_FW(Vs[i], x0s[i], eps, 60), i)
    assert b.calls[0] == (0, 7, (True, True, True)) and all(c[2][1] is False for c in b.calls[1:])


# ------------------------------------------------------------------------------------------------- staggered stops
STAGGER = dict(m=8, n=40, eps=1e-2, maxitrs=400, seeds=(301, 302, 303, 304, 305))


@pytest.fixture(scope="module")
def stagger():
    c = STAGGER
    Vs = [gaussian_design(c["m"], c["n"], s) for s in c["seeds"]]
    x0 = np.ones(c["n"]) / c["n"]
    single = [run_away(NumpyRun(V, x0), c["eps"], c["maxitrs"], 64, R=0) for V in Vs]
    return Vs, x0, single


def test_the_staggered_instances_stop_where_the_oracle_stops(stagger):
    Vs, x0, single = stagger
    c = STAGGER
    stops = [len(O.D_opt_FW_away(V, x0, c["eps"], c["maxitrs"])[1]) - 1 for V in Vs]
    assert stops == [58, 65, 52, 59, 66]
    assert [len(r[1]) - 1 for r in single] == stops


@pytest.mark.parametrize("S,R", [(64, 0), (7, 0), (None, None), (7, None), (1, 5)])
def test_staggered_stops_inside_a_chunk(stagger, S, R):
    """An instance that stops idles through the rest of its chunk (the stand-in, like the device, ends its records
    there) and is dropped from the active set of the next; the others run on, and every instance equals its own
    single replay."""
    Vs, x0, single = stagger
    c = STAGGER
    b = NumpyBatch(Vs, [x0] * len(Vs))
    res = batch_away(b, c["eps"], c["maxitrs"], S, R=R)
    stops = [len(r[1]) - 1 for r in single]
    for i in range(b.K):
        want = single[i] if R == 0 else run_away(NumpyRun(Vs[i], x0), c["eps"], c["maxitrs"], S, R=R)
        assert len(want[1]) - 1 == stops[i]
        _same(res[i], want, (i, S, R))
        assert b.inst[i].k == stops[i]                          # no update behind the stop
    mixed = 0
    for first, nsteps, active in b.calls:
        # active: exactly the instances whose stop lies at or behind the chunk's first iteration
        assert active == tuple(stops[i] >= first for i in range(b.K))
        inside = [first <= stops[i] < first + nsteps for i in range(b.K) if active[i]]
        mixed += any(inside) and not all(inside)
    assert mixed >= 1                                           # a call held both: otherwise this shows nothing
    if (S, R) == (64, 0):
        assert [a for _, _, a in b.calls] == [(True,) * 5, (False, True, False, False, True)]
    assert b.calls[-1][0] <= max(stops) < b.calls[-1][0] + b.calls[-1][1]       # no call behind the last stop
    for k, active in b.snaps:
        assert active == tuple(stops[i] >= k for i in range(b.K))


# ------------------------------------------------------------------------------------------------------- chunk cuts
@pytest.mark.parametrize("R", [0, 1, 5, 16])
@pytest.mark.parametrize("S", [None, 1, 7, 64])
def test_chunks_end_before_the_anchors(R, S):
    Vs, x0s = _axis_batch()
    maxitrs = 37
    b = NumpyBatch(Vs, x0s)
    res = batch_away(b, -1.0, maxitrs, S, R=R)
    want = (R if R > 0 else 64) if S is None else S
    k = 0
    for first, nsteps, active in b.calls:
        assert first == k and nsteps >= 1 and all(active)
        room = maxitrs - k if R == 0 else min(maxitrs - k, R - k % R)
        assert nsteps == min(want, room)
        if R > 0:
            assert not any(j % R == 0 for j in range(k + 1, k + nsteps))      # no anchor inside the chunk
        k += nsteps
    assert k == maxitrs
    assert [s[0] for s in b.snaps] == ([] if R == 0 else list(range(0, maxitrs, R)))
    for i in range(b.K):
        assert len(res[i][1]) == maxitrs
        assert b.inst[i].calls == [(c[0], c[1]) for c in b.calls]
        assert b.inst[i].snaps == [s[0] for s in b.snaps]
        _same(res[i], run_away(NumpyRun(Vs[i], x0s[i]), -1.0, maxitrs, 1, R=R), (i, R, S))


def test_chunks_of_the_frank_wolfe_variant():
    Vs, x0s = _axis_batch()
    for S, calls in ((1, [(k, 1) for k in range(10)]), (7, [(0, 7), (7, 3)]), (64, [(0, 10)])):
        b = NumpyBatch(Vs, x0s)
        gen = _alg()._fw_batch_device_steps(b, b.logdet, [-1.0] * b.K, 10, S, 0.0)
        yielded = []
        try:
            while True:
                yielded.append(next(gen))
        except StopIteration as stop:
            res = stop.value
        assert [(c[0], c[1]) for c in b.calls] == calls and all(len(r[1]) == 10 for r in res)
        assert yielded == [first + nsteps - 1 for first, nsteps in calls]       # the last k of each chunk
    with pytest.raises(ValueError):
        batch_fw(NumpyBatch(Vs, x0s), -1.0, 10, 0)


# ----------------------------------------------------------------------------------------------------------- guard
@pytest.mark.parametrize("away", [0, 1])
@pytest.mark.parametrize("field", ["hcoef", "p", "xscale", "xadd", "hdiv"])
def test_a_tampered_record_raises_naming_the_instance(away, field):
    Vs, x0s = _axis_batch()
    b = NumpyBatch(Vs, x0s)
    probe = NumpyRun(Vs[1], x0s[1]).run(away, -1.0, 12)[11]
    wrong = probe.p + 1 if field == "p" else float(np.nextafter(getattr(probe, field), INF))
    b.inst[1].tamper = (11, field, wrong)
    solver = batch_away if away else batch_fw
    with pytest.raises(RuntimeError, match=r"instance 1: iteration 11: field %s " % field):
        solver(b, -1.0, 60, 7)
    b = NumpyBatch(Vs, x0s)
    b.inst[2].tamper = (0, "status", 1)
    with pytest.raises(RuntimeError, match=r"instance 2: iteration 0: .*field status"):
        solver(b, -1.0, 60, 7)


def test_a_pivot_outside_the_columns_raises_the_update_error():
    """Status 2 on instance 2 at k = 9: the replay reaches the record in its turn and raises what the sequential
    solver's update raises; no update was applied to that instance."""
    Vs, x0s = _axis_batch()
    b = NumpyBatch(Vs, x0s)
    b.inst[2].plant = (9, N.Probe(0, INT64_MAX, NAN, INF, 0.0))
    with pytest.raises(ValueError, match="instance 2, iteration 9: accbpg_fw_update: bad argument"):
        batch_away(b, -1.0, 60, 7, R=0)
    # no further chunk is enqueued for anybody behind the record
    assert b.inst[2].k == 9 and [(c[0], c[1]) for c in b.calls] == [(0, 7), (7, 7)]
    ref = NumpyRun(Vs[2], x0s[2])
    ref.run(1, -1.0, 9)
    np.testing.assert_array_equal(b.inst[2].x(), ref.x())
    np.testing.assert_array_equal(b.inst[2].H, ref.H)


# ------------------------------------------------------------------------------------------ names, signatures, ABI
def test_public_names_and_signatures():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import D_opt_alg, batched
    plain = "(batch, x0, eps, maxitrs, sync_every=64)"
    away = "(batch, x0, eps, maxitrs, sync_every=None, logdet_refresh=None, logdet_ring=None)"
    for name in ("D_opt_FW_batch_device", "D_opt_FW_away_batch_device"):
        assert name in acc.__all__ and callable(getattr(acc, name))
    assert str(inspect.signature(acc.D_opt_FW_batch_device)) == plain
    assert str(inspect.signature(acc.D_opt_FW_away_batch_device)) == away
    assert str(inspect.signature(D_opt_alg.D_opt_FW_batch_device_steps)) == plain
    assert str(inspect.signature(D_opt_alg.D_opt_FW_away_batch_device_steps)) == away
    assert inspect.isgeneratorfunction(D_opt_alg._fw_batch_device_steps)
    assert inspect.isgeneratorfunction(D_opt_alg._away_batch_device_steps)
    assert str(inspect.signature(batched.DOptimalBatch.fw_run)) == "(self, away, eps, nsteps, active=None)"
    # one copy of the decisions and of the guard
    for fn, text in ((D_opt_alg._fw_batch_device_steps, "_fw_decide("), (D_opt_alg._away_batch_device_steps, "_AwayRun("),
                     (D_opt_alg._away_batch_device_steps, "_chunk("), (D_opt_alg._guard_instance, "_guard(")):
        assert text in inspect.getsource(fn)


def test_the_entry_is_declared_bound_and_exported_and_the_abi_version_stays():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    assert "accbpg_dopt_batch_fw_run" in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _lib.load()
    assert "accbpg_dopt_batch_fw_run" in _lib.EXPORTS and hasattr(lib, "accbpg_dopt_batch_fw_run")
    assert lib.accbpg_abi_version() == 3
    # the records cross the C-ABI as they do for accbpg_fw_run: 96 bytes each, row i = instance i
    import ctypes as C
    assert C.sizeof(_lib.FwStep) == 96
