"""The host side of D_opt_FW_device / D_opt_FW_away_device without a GPU: the replay of the records of
``accbpg_fw_run`` through the solvers' one copy of the decisions, the bit-for-bit guard, and where the chunks are cut.

The records come from ``NumpyRun``: a stand-in for the handle that keeps (x, w, H) in NumPy, steps them with
tests/fw_numpy.py's one-step restatement, and takes the decisions of an iteration as include/accbpg_hip.h states them
for the device (written out here a second time, in Python floats -- so the guard compares two texts, not one with
itself).  Like the device it stops in mid-chunk, and reports a pivot outside [0, n) with status 2."""
import numpy as np
import pytest

import fw_numpy as N
from conftest import gaussian_design
from oracle import np_oracle as O

INT64_MAX = 2 ** 63 - 1
NAN, INF = float("nan"), float("inf")
APPLIED, STOPPED, BAD_PIVOT = 0, 1, 2


def _alg():
    from accbpg_and_fw_amd import D_opt_alg
    return D_opt_alg


class Rec:
    """accbpg_fw_step"""

    def __init__(self, pr, q_prev):
        self.i, self.j, self.w_i, self.w_j, self.x_j, self.q_prev = pr.i, pr.j, pr.w_i, pr.w_j, pr.x_j, q_prev
        self.p, self.xscale, self.xadd, self.hcoef, self.hdiv = -1, 0.0, 0.0, 0.0, 0.0
        self.kind, self.status = -1, STOPPED


def _div(a, b):
    """IEEE division (the device's), where Python raises"""
    return float(np.float64(a) / np.float64(b))


def device_decision(rec, m, n, away, eps):
    """include/accbpg_hip.h, accbpg_fw_run"""
    w_i, w_j, x_j = rec.w_i, rec.w_j, rec.x_j
    eps_pos = w_i / m - 1
    eps_neg = 1 - w_j / m
    if eps_pos <= eps and eps_neg <= eps:
        return rec
    with np.errstate(all="ignore"):
        if not away or eps_pos >= eps_neg:
            t = _div(w_i / m - 1, w_i - 1)
            coef = _div(t, 1 - t + t * w_i) if away else _div(t, 1 + t * (w_i - 1))
            rec.p, rec.xscale, rec.xadd, rec.hcoef, rec.hdiv, rec.kind = rec.i, 1 - t, t, -coef, 1 - t, 0
        else:
            a = _div(1 - w_j / m, w_j - 1)
            b = _div(x_j, 1 - x_j)
            t = b if b < a else a
            coef = _div(t, 1 + t - t * w_j)
            rec.p, rec.xscale, rec.xadd, rec.hcoef, rec.hdiv, rec.kind = rec.j, 1 + t, -t, coef, 1 + t, 1
    rec.status = APPLIED if 0 <= rec.p < n else BAD_PIVOT
    return rec


class NumpyRun:
    """What the device solvers ask of their state object, in NumPy."""

    def __init__(self, V, x0):
        self.V = V
        self.m, self.n = V.shape
        self._x, det, self.H, self.w = N.setup_f64(V, x0)
        self.logdet_gram = float(np.log(det))
        self.q_prev = 0.0
        self.k = 0                  # iterations applied so far
        self.calls = []             # (first iteration, nsteps) of every run call
        self.snaps = []             # iterations at which a snapshot was taken
        self.ring, self.depth = [], 1
        self.tamper = None          # (k, field, value): falsify one record
        self.plant = None           # (k, probe): replace the probe record of iteration k

    def logdet_ring(self, depth):
        self.depth, self.ring = depth, []

    def snapshot(self):
        value = self.ring.pop(0) if len(self.ring) >= self.depth else NAN
        self.ring.append(float(np.log(np.linalg.det(self.H))))          # np_oracle.D_opt_FW_away, F[k]
        self.snaps.append(self.k)
        return value

    def flush_logdet(self):
        return self.ring.pop(0) if self.ring else NAN

    def run(self, away, eps, nsteps):
        self.calls.append((self.k, nsteps))
        out = []
        for _ in range(nsteps):
            pr = N.probe(self.w, self._x, away)
            if self.plant is not None and self.plant[0] == self.k:
                pr = self.plant[1]
            rec = device_decision(Rec(pr, self.q_prev), self.m, self.n, away, eps)
            applied = rec.status == APPLIED
            if self.tamper is not None and self.tamper[0] == self.k:
                setattr(rec, self.tamper[1], self.tamper[2])         # (the record only: the state goes its own way)
            out.append(rec)
            if not applied:
                break                                   # the later records of the chunk read "not run"
            v = self.V[:, rec.p]
            self.q_prev = float(np.dot(v, np.dot(self.H, v)))
            self._x = N.update_x(self._x, rec.p, rec.xscale, rec.xadd)
            self.H, self.w = N.update_f64(self.V, self.H, self.w, rec.p, rec.hcoef, rec.hdiv)
            self.k += 1
        return out

    def bad_pivot(self):
        raise ValueError("accbpg_fw_update: bad argument (pivot index outside [0, n))")

    def x(self):
        return self._x.copy()


def _drain(gen):
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def run_fw(st, eps, maxitrs, S):
    return _drain(_alg()._fw_device_steps(st, eps, maxitrs, False, 1, S, 0.0))


def run_away(st, eps, maxitrs, S, R=None, ring=None):
    return _drain(_alg()._away_device_steps(st, eps, maxitrs, False, 1, S, R, ring, 0.0))


def _axis(m=8, n=40, start=0):
    s, x0 = N.axis_run_design(m, n, start)
    V, G = N.axis_design(m, n, s, x0)
    return V, x0


# ------------------------------------------------------------------------------------------ replay against the oracle
@pytest.mark.parametrize("S", [1, 7, 64])
@pytest.mark.parametrize("eps", [-1.0, 1.0])
def test_replay_is_the_oracle_bit_for_bit_on_an_axis_design(S, eps):
    """(8, 40), 60 iterations; eps = 1 stops both solvers before the chunks run out.  F of the away variant with a factorisation per
    iteration (logdet_refresh = 1, the reference's computation) is the oracle's expression on the oracle's H."""
    V, x0 = _axis()
    xo, Fo, SPo, SNo, _ = O.D_opt_FW(V, x0, eps, 60)
    x, F, SP, SN, T = run_fw(NumpyRun(V, x0), eps, 60, S)
    assert len(F) == len(Fo) and (eps < 0 or 2 < len(F) < 60)
    for a, b in ((x, xo), (F, Fo), (SP, SPo), (SN, SNo)):
        np.testing.assert_array_equal(a, b)
    xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, eps, 60)
    for ring in (1, 3):
        x, F, SP, SN, T = run_away(NumpyRun(V, x0), eps, 60, S, R=1, ring=ring)
        assert len(F) == len(Fo) and (eps < 0 or 2 < len(F) < 60)
        for a, b in ((x, xo), (F, Fo), (SP, SPo), (SN, SNo)):
            np.testing.assert_array_equal(a, b)
    for R in (0, 5, 16):            # F by the determinant lemma between the anchors: test_fw_step_cpu's bar for F
        x, F, SP, SN, T = run_away(NumpyRun(V, x0), eps, 60, S, R=R)
        for a, b in ((x, xo), (SP, SPo), (SN, SNo)):
            np.testing.assert_array_equal(a, b)
        assert np.all(np.isfinite(F)) and np.max(np.abs(F - Fo)) <= 1e-12 * (1 + np.max(np.abs(Fo)))


def test_replay_stops_where_the_records_stop():
    """A stop at k = 3 mod 7 with S = 7 and a stop at k = 0: the replay runs no further chunk."""
    V, x0 = _axis()
    xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, -1.0, 60)
    k_stop = 10                                          # 10 = 3 mod 7
    eps = max(SPo[k_stop], SNo[k_stop])
    assert all(max(SPo[k], SNo[k]) > eps for k in range(k_stop))
    st = NumpyRun(V, x0)
    x, F, SP, SN, T = run_away(st, eps, 60, 7, R=0)
    assert len(F) == k_stop + 1 and st.calls == [(0, 7), (7, 7)] and st.k == k_stop
    np.testing.assert_array_equal(SP, SPo[:k_stop + 1])
    np.testing.assert_array_equal(x, O.D_opt_FW_away(V, x0, eps, 60)[0])
    for solver in (run_fw, run_away):
        st = NumpyRun(V, x0)
        x, F, SP, SN, T = solver(st, 1e30, 60, 7)
        assert len(F) == 1 and st.calls == [(0, 7)] and st.k == 0
        np.testing.assert_array_equal(x, x0)


def test_replay_follows_the_oracle_on_a_gaussian_design():
    """(30, 1000) seed 10, the bars of test_fw_step_cpu.test_chain_follows_the_oracle_on_gaussian_designs"""
    V = gaussian_design(30, 1000, 10)
    x0 = np.ones(1000) / 1000
    xo, Fo, SPo, SNo, _ = O.D_opt_FW(V, x0, 1e-6, 200)
    x, F, SP, SN, T = run_fw(NumpyRun(V, x0), 1e-6, 200, 64)
    assert len(F) == len(Fo) and np.max(np.abs(x - xo)) < 1e-9
    for a, b in ((F, Fo), (SP, SPo), (SN, SNo)):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9)
    xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, 1e-6, 200)
    x, F, SP, SN, T = run_away(NumpyRun(V, x0), 1e-6, 200, None)
    assert abs(len(F) - len(Fo)) <= 2
    k = min(len(F), len(Fo))
    assert np.max(np.abs(x - xo)) < 1e-8
    np.testing.assert_allclose(F[:k], Fo[:k], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(SP[:k], SPo[:k], rtol=1e-8, atol=1e-8)


# ----------------------------------------------------------------------------------------------------------- guard
@pytest.mark.parametrize("away", [0, 1])
@pytest.mark.parametrize("field", ["hcoef", "p", "xscale", "xadd", "hdiv"])
def test_a_tampered_record_raises(away, field):
    V, x0 = _axis()
    st = NumpyRun(V, x0)
    probe = NumpyRun(V, x0).run(away, -1.0, 12)[11]
    wrong = probe.p + 1 if field == "p" else float(np.nextafter(getattr(probe, field), INF))
    st.tamper = (11, field, wrong)
    solver = run_away if away else run_fw
    with pytest.raises(RuntimeError, match=r"iteration 11: field %s " % field):
        solver(st, -1.0, 60, 7)
    # the sign of a zero is a bit, too
    st = NumpyRun(V, x0)
    st.tamper = (0, "xadd", -0.0)
    st.plant = (0, N.Probe(3, 5, 8.0, 8.0, 0.25))       # w_i = m: t = 0 exactly, a Frank-Wolfe step of length 0
    with pytest.raises(RuntimeError, match="iteration 0: field xadd "):
        solver(st, -1.0, 60, 7)


def test_a_disagreement_about_the_stop_raises():
    V, x0 = _axis()
    for status, eps in ((STOPPED, -1.0), (APPLIED, 1e30)):
        st = NumpyRun(V, x0)
        st.tamper = (0, "status", status)
        with pytest.raises(RuntimeError, match="iteration 0: .*field status"):
            run_fw(st, eps, 60, 7)


def test_a_pivot_outside_the_columns_raises_the_update_error():
    """Status 2: a NaN w_i fails both comparisons (no stop, away branch) and the away index of an empty support is
    INT64_MAX.  The replay reaches the record in its turn -- the iterations before it are kept -- and raises what the
    sequential solver's update raises; no update was applied."""
    V, x0 = _axis()
    st = NumpyRun(V, x0)
    st.plant = (9, N.Probe(0, INT64_MAX, NAN, INF, 0.0))
    with pytest.raises(ValueError, match="accbpg_fw_update: bad argument"):
        run_away(st, -1.0, 60, 7, R=0)
    assert st.k == 9 and st.calls == [(0, 7), (7, 7)]
    ref = NumpyRun(V, x0)
    ref.run(1, -1.0, 9)
    np.testing.assert_array_equal(st.x(), ref.x())
    np.testing.assert_array_equal(st.H, ref.H)


def test_nan_compares_as_in_python():
    """NaN in w_j alone: the stop test fails, eps_pos >= NaN fails, the away branch computes NaN scalars -- the guard
    takes NaN for NaN (payloads are not compared) and the step is applied."""
    V, x0 = _axis()
    st = NumpyRun(V, x0)
    st.plant = (2, N.Probe(3, 5, 9.0, NAN, 0.25))
    x, F, SP, SN, T = run_away(st, -1.0, 4, 7, R=0)
    assert len(F) == 4 and np.isnan(SN[2]) and np.all(np.isnan(x))


# ------------------------------------------------------------------------------------------------------- chunk cuts
@pytest.mark.parametrize("R", [0, 1, 5, 16])
@pytest.mark.parametrize("S", [None, 1, 7, 64])
def test_chunks_end_before_the_anchors(R, S):
    alg = _alg()
    V, x0 = _axis()
    maxitrs = 37
    st = NumpyRun(V, x0)
    x, F, SP, SN, T = run_away(st, -1.0, maxitrs, S, R=R)
    want = (R if R > 0 else 64) if S is None else S
    k = 0
    for first, nsteps in st.calls:
        assert first == k and nsteps >= 1
        room = maxitrs - k if R == 0 else min(maxitrs - k, R - k % R)
        assert nsteps == min(want, room)
        if R > 0:
            assert not any(j % R == 0 for j in range(k + 1, k + nsteps))      # no anchor inside the chunk
        k += nsteps
    assert k == maxitrs == len(F)
    assert st.snaps == ([] if R == 0 else list(range(0, maxitrs, R)))
    one = NumpyRun(V, x0)
    x1, F1, SP1, SN1, T1 = run_away(one, -1.0, maxitrs, 1, R=R)
    for a, b in ((x, x1), (F, F1), (SP, SP1), (SN, SN1)):
        np.testing.assert_array_equal(a, b)
    assert alg._chunk(0, 5000, 4000) == 1024 and alg._chunk(32, 100, None, 16) == 16 and alg._chunk(35, 100, 64, 16) == 13
    with pytest.raises(ValueError):
        alg._chunk(0, 10, 0)


def test_chunks_of_the_frank_wolfe_variant():
    V, x0 = _axis()
    for S, calls in ((1, [(k, 1) for k in range(10)]), (7, [(0, 7), (7, 3)]), (64, [(0, 10)])):
        st = NumpyRun(V, x0)
        x, F, SP, SN, T = run_fw(st, -1.0, 10, S)
        assert st.calls == calls and len(F) == 10


def test_public_names_and_signatures():
    import inspect

    import accbpg_and_fw_amd as acc
    assert str(inspect.signature(acc.D_opt_FW_device)) == \
        "(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=64)"
    assert str(inspect.signature(acc.D_opt_FW_away_device)) == \
        "(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=None, logdet_refresh=None, logdet_ring=None)"
    from accbpg_and_fw_amd import D_opt_alg
    assert inspect.isgeneratorfunction(D_opt_alg._fw_device_steps) and hasattr(D_opt_alg, "D_opt_FW_away_device_steps")
