"""The host side of D_opt_FW_div_step_device / D_opt_FW_descent_step_device without a GPU: where the chunks are cut,
the replay of the records of ``accbpg_fw_div_run`` through the solvers' one copy of the decisions, the roll-back on a
disagreement and the hand-backs.

The records come from ``NumpyDiv``: a stand-in for the handle that keeps (x, w, H) in tests/fwdiv_numpy.py's State and
predicts the decisions of an iteration as include/accbpg_hip.h states them for the device -- written out here a second
time, so the replay compares two texts, not one with itself.  Like the device it applies what IT decided, stops in
mid-chunk and hands back; on request it flips one acceptance or moves one step length by an ulp, and its state then goes
the wrong way until the host restores it."""
import math
import time
import types

import numpy as np
import pytest

import fwdiv_numpy as R
from conftest import gaussian_design

FILL, FLOOR, TRIALS_MAX = 1e-15, 1e-6, 64
LINESEARCH, FIXED_L, CLASSICAL = 0, 1, 2
APPLIED, STOPPED, HANDED_BACK = 0, 1, 2
BUDGET, L_INF, SLOPE, MIN_X, PIVOT, CAP, ARITH = range(1, 8)
RAISES = (ZeroDivisionError, OverflowError, ValueError, TypeError)


def _alg():
    from accbpg_and_fw_amd import D_opt_alg
    return D_opt_alg


def _housing():
    import os
    from oracle import np_oracle as O
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    X, _ = O.load_libsvm_file(os.path.join(root, "tests", "golden", "data", "housing.txt"))
    return np.ascontiguousarray(X.T if X.shape[0] > X.shape[1] else X, dtype=np.float64)     # D_opt_libsvm's matrix


DESIGNS = {}


def design(name):
    if name not in DESIGNS:
        DESIGNS[name] = _housing() if name == "housing" else gaussian_design(30, 1000, 12)
    V = DESIGNS[name]
    return V, np.ones(V.shape[1]) / V.shape[1]


def scalars(a, rec, ld, q, m, radius):
    """(hcoef, hdiv, ld1, q1, f1) as the header states them for the device"""
    tau = a * (radius - FILL) / (1 - a)
    den = 1 + tau * rec.w_i
    hcoef, hdiv = -tau / den, 1 - a
    ld1 = ld + m * math.log(hdiv) + math.log(den)
    q1 = q + a * (FILL - q)
    return hcoef, hdiv, ld1, q1, -ld1 - q1 * ((rec.sum_w + hcoef * rec.sum_u2) / hdiv)


def predict(rec, n, bk, L, mode, gamma, ls_ratio, eps, k, flip=None):
    """include/accbpg_hip.h, accbpg_fw_div_run, modes 0 and 1: (status, reason, L, trials, a, hcoef, hdiv, ld1, q1, f1)"""
    fx = -bk.ld - bk.q * rec.sum_w
    if not 0 <= rec.i < n:
        return HANDED_BACK, PIVOT
    div = rec.div if rec.div != 0 else FLOOR
    slope = 0.0 if 0 < rec.slope <= FLOOR else rec.slope
    if slope > 0:
        return HANDED_BACK, SLOPE
    if not rec.min_x > 0:
        return HANDED_BACK, MIN_X
    if mode == LINESEARCH:
        L = L / ls_ratio
    try:
        for t in range(TRIALS_MAX):
            r = (-slope / (2 * L * div)) ** (1 / (gamma - 1))
            a = 1.0 if 1.0 < r else r
            if not a < 1:
                return HANDED_BACK, CAP
            if flip == "ulp":
                a = float(np.nextafter(a, 0.0))
            hcoef, hdiv, ld1, q1, f1 = scalars(a, rec, bk.ld, bk.q, bk.m, bk.radius)
            if mode != LINESEARCH:
                break
            if math.isinf(L):
                return HANDED_BACK, L_INF
            accept = f1 <= fx + a * slope + a ** gamma * L * div
            if flip == "accept" and t == 0:
                accept = not accept
            if accept:
                break
            L = L * ls_ratio
        else:
            return HANDED_BACK, BUDGET
    except RAISES:
        return HANDED_BACK, ARITH
    stop = k > 0 and abs(fx - bk.F_prev) < eps
    bk.ld, bk.q, bk.F_prev = ld1, q1, fx
    return (STOPPED if stop else APPLIED), 0, L, t + 1, a, hcoef, hdiv, ld1, q1, f1


class NumpyDiv:
    """What the device solvers ask of their state object, in NumPy."""

    def __init__(self, V, x0, radius=1, refresh=256):
        self.s = R.State(V, x0)
        self.V, self.m, self.n, self.radius = self.s.V, self.s.m, self.s.n, float(radius)
        self.book = _alg()._DivBook(self.m, radius, refresh, self.s.ld)
        self.pending = None
        self.k = 0                  # rank-one steps applied since the start, roll-backs undone
        self.calls = []             # (k0, nsteps, book.since) of every run call
        self.flips = {}             # k0 + j -> "accept" | "ulp" | "stop": falsify the prediction of that iteration
        self.plant = {}             # steps applied so far -> fields to overwrite in the record of a probe there
        self.reinits = 0

    # -- the step-by-step entries
    def _record(self):
        d = self.s.probe(self.radius)
        d.update(self.plant.get(self.k, {}))
        return d

    def probe_div(self):
        d = self._record()
        if not 0 <= d["i"] < self.n:
            self.bad_div_pivot()
        self.pending = d
        return types.SimpleNamespace(**{k: v for k, v in d.items() if k not in ("hv", "u")})

    def apply_step(self, p, a, hcoef, hdiv):
        assert self.pending is not None and self.pending["i"] == p, "accbpg_fw_div_apply: no probe pending"
        self.s.apply(self.pending, a, self.radius, hcoef, hdiv)
        self.pending = None
        self.k += 1

    def refresh_if_due(self):
        if self.book.refresh_due():
            self.reinit(self.s.x)

    def reinit(self, x):
        self.s.init(np.array(x))
        self.book.reset(self.s.ld)
        self.pending = None
        self.reinits += 1

    def capped(self, rec, valued):
        vertex = np.full(self.n, FILL)
        vertex[rec.i] = self.radius
        trial = self.s.x + 1.0 * (vertex - self.s.x)
        return trial, (R._value(self.V, trial) if valued else None)

    def bad_div_pivot(self):
        raise ValueError("accbpg_fw_div_probe_step: bad argument (pivot index outside [0, n))")

    def x(self):
        return self.s.x.copy()

    # -- what the device form adds
    def snapshot(self):
        self.saved = (self.s.x.copy(), self.s.w.copy(), self.s.H.copy(), self.k)

    def restore(self):
        self.s.x, self.s.w, self.s.H = (v.copy() for v in self.saved[:3])
        self.k = self.saved[3]
        self.pending = None

    def run_div(self, mode, L, gamma, ls_ratio, epsilon, k0, F_prev, nsteps):
        assert 1 <= nsteps <= 1024
        self.calls.append((k0, nsteps, self.book.since))
        bk = types.SimpleNamespace(ld=self.book.ld, q=self.book.q, m=self.m, radius=self.radius, F_prev=F_prev)
        out, flipped = [], False
        if mode == CLASSICAL:
            assert self.pending is not None and k0 >= 1, "accbpg_fw_div_run: no probe pending"
        for j in range(nsteps):
            k = k0 + j
            # (one per call: what follows a falsified record is thrown away by the host, a flip there would be lost)
            flip = self.flips.pop(k, None) if not flipped else None
            flipped = flipped or flip is not None
            r = types.SimpleNamespace(L=0.0, trials=0, a=0.0, hcoef=0.0, hdiv=0.0, ld1=bk.ld, q1=bk.q, f1=0.0, reason=0)
            if mode == CLASSICAL:
                prev = types.SimpleNamespace(**self.pending)
                a = 2 / (k + 2)
                if flip == "ulp":
                    a = float(np.nextafter(a, 0.0))
                r.a, r.hcoef, r.hdiv, bk.ld, bk.q, _ = (a,) + scalars(a, prev, bk.ld, bk.q, bk.m, bk.radius)
                r.ld1, r.q1 = bk.ld, bk.q
                self.apply_step(prev.i, r.a, r.hcoef, r.hdiv)
                d = self._record()
                self.pending = d
                r.probe = types.SimpleNamespace(**{f: v for f, v in d.items() if f not in ("hv", "u")})
                r.f1 = -bk.ld - bk.q * d["sum_w"]
                stop = abs(r.f1 - bk.F_prev) < epsilon or math.sqrt(d["sum_w2"]) < epsilon
                bk.F_prev = r.f1
                if flip == "stop":
                    stop = not stop
                r.status = STOPPED if stop else APPLIED
                out.append(r)
                if stop:
                    break
                continue
            d = self._record()
            r.probe = types.SimpleNamespace(**{f: v for f, v in d.items() if f not in ("hv", "u")})
            res = predict(r.probe, self.n, bk, L, mode, gamma, ls_ratio, epsilon, k, flip)
            r.status, r.reason = res[:2]
            out.append(r)
            self.pending = d if 0 <= d["i"] < self.n else None
            if r.status == HANDED_BACK:
                break
            L, r.trials, r.a, r.hcoef, r.hdiv, r.ld1, r.q1, r.f1 = res[2:]
            r.L = L
            if flip == "stop":
                r.status = STOPPED if r.status == APPLIED else APPLIED
            self.apply_step(d["i"], r.a, r.hcoef, r.hdiv)
            if r.status == STOPPED:
                break
        return out


def device_div(V, x0, L, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1, refresh=256,
               sync_every=64, prepare=None):
    D = _alg()
    st = NumpyDiv(V, x0, radius, refresh)
    if prepare:
        prepare(st)
    run = D._DivStepRun(st.book, L, maxitrs, gamma, epsilon, linesearch, ls_ratio)
    stats = D._device_stats(None)
    out = D._drain(D._div_device_steps(st, run, maxitrs, False, 1, sync_every, stats, time.time()))
    return out, stats, st


def sequential_div(V, x0, L, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1, refresh=256,
                   prepare=None):
    """The loop of D_opt_FW_div_step_steps on the stand-in (for the runs fwdiv_numpy cannot plant a record into)."""
    D = _alg()
    st = NumpyDiv(V, x0, radius, refresh)
    if prepare:
        prepare(st)
    run = D._DivStepRun(st.book, L, maxitrs, gamma, epsilon, linesearch, ls_ratio)
    for k in range(maxitrs):
        st.refresh_if_due()
        rec = st.probe_div()
        step, trial, stop = run.decide(k, rec, 0.0, lambda r: st.capped(r, linesearch))
        if trial is None:
            st.apply_step(*step)
        else:
            st.reinit(trial)
        if stop:
            break
    return run.result(st.x())


def device_descent(V, x0, maxitrs, epsilon=1e-14, radius=1, refresh=256, sync_every=64, prepare=None):
    D = _alg()
    st = NumpyDiv(V, x0, radius, refresh)
    if prepare:
        prepare(st)
    run = D._DescentRun(st.book, maxitrs, epsilon)
    stats = D._device_stats(None)
    out = D._drain(D._descent_device_steps(st, run, maxitrs, False, 1, sync_every, stats, time.time()))
    return out, stats, st


def same(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


@pytest.fixture(scope="module")
def refs():
    """The sequential restatement's runs, computed once and left unchanged."""
    out = {}
    for name in ("housing", "gauss"):
        V, x0 = design(name)
        for refresh in (0, 1, 5, 256):
            out[name, "div", refresh] = R.fw_div_step(V, 1.0, x0, 150, 2.0, refresh=refresh)
            out[name, "descent", refresh] = R.fw_descent_step(V, x0, 150, refresh=refresh)
    return out


@pytest.mark.parametrize("name", ["housing", "gauss"])
@pytest.mark.parametrize("refresh", [0, 1, 5, 256])
@pytest.mark.parametrize("S", [1, 7, 64])
def test_whole_runs_and_chunk_cuts(refs, name, refresh, S):
    V, x0 = design(name)
    (x, F, Ls, T), stats, st = device_div(V, x0, 1.0, 150, 2.0, refresh=refresh, sync_every=S)
    same((x, F, Ls), refs[name, "div", refresh])
    assert len(T) == len(F) and stats["rollbacks"] == 0 and stats["handed_back"] == 0
    for k0, nsteps, since in st.calls:                          # no chunk spans a refresh
        assert 1 <= nsteps <= S and (not refresh or since + nsteps <= refresh)
    assert sum(c[1] for c in st.calls) == len(F) and stats["chunks"] == len(st.calls)
    if S == 64 and refresh in (0, 256):
        assert [c[:2] for c in st.calls] == [(0, 64), (64, 64), (128, 22)]
    (x, F, T, G), stats, st = device_descent(V, x0, 150, refresh=refresh, sync_every=S)
    same((x, F), refs[name, "descent", refresh])
    assert len(T) == len(G) == len(F) and not G.any() and stats["rollbacks"] == 0
    for k0, nsteps, since in st.calls:                          # ... nor ends on the step that makes one due
        assert 1 <= nsteps <= S and (not refresh or since + nsteps < refresh)
    if refresh == 1:
        assert st.calls == []
    if refresh == 5:
        assert st.reinits == 149 // 5


@pytest.mark.parametrize("kind", ["accept", "ulp", "stop"])
@pytest.mark.parametrize("planted", [(7,), (10,), (13,), (10, 11), (0, 7, 10, 13, 14, 149)], ids=str)
def test_planted_disagreements_div(refs, kind, planted):
    """First (7), a middle (10) and the last (13) record of a chunk of 7, and two consecutive iterations."""
    V, x0 = design("gauss")
    (x, F, Ls, T), stats, st = device_div(V, x0, 1.0, 150, 2.0, sync_every=7,
                                          prepare=lambda s: s.flips.update({k: kind for k in planted}))
    same((x, F, Ls), refs["gauss", "div", 256])
    assert stats["rollbacks"] == len(planted) and st.flips == {} and st.k == len(F)


@pytest.mark.parametrize("kind", ["ulp", "stop"])
@pytest.mark.parametrize("planted", [(8,), (10,), (14,), (10, 11), (1, 8, 10, 14, 15, 149)], ids=str)
def test_planted_disagreements_descent(refs, kind, planted):
    V, x0 = design("gauss")
    (x, F, T, G), stats, st = device_descent(V, x0, 150, sync_every=7,
                                             prepare=lambda s: s.flips.update({k: kind for k in planted}))
    same((x, F), refs["gauss", "descent", 256])
    assert stats["rollbacks"] == len(planted) and st.flips == {}


def _stop_epsilon(F, kstop):
    d = np.abs(np.diff(F))
    lo = d[:kstop - 1].min() if kstop > 1 else np.inf
    return None if not d[kstop - 1] < lo else float((d[kstop - 1] + min(lo, 2 * d[kstop - 1] + 1.0)) / 2)


def test_stop_in_mid_chunk(refs):
    V, x0 = design("gauss")
    F = refs["gauss", "div", 256][1]
    kstop, eps = next((k, _stop_epsilon(F, k)) for k in range(10, 140, 7) if _stop_epsilon(F, k) is not None)
    want = R.fw_div_step(V, 1.0, x0, 150, 2.0, epsilon=eps)
    assert len(want[1]) == kstop + 1 and kstop % 7 == 3
    (x, F, Ls, T), stats, st = device_div(V, x0, 1.0, 150, 2.0, epsilon=eps, sync_every=7)
    same((x, F, Ls), want)
    assert stats["rollbacks"] == 0 and st.calls[-1][:2] == (kstop - 3, 7) and st.k == kstop + 1
    F = refs["gauss", "descent", 256][1]
    kstop, eps = next((k, _stop_epsilon(F, k)) for k in range(11, 140, 7) if _stop_epsilon(F, k) is not None)
    want = R.fw_descent_step(V, x0, 150, epsilon=eps)
    assert len(want[1]) == kstop + 1
    (x, F, T, G), stats, st = device_descent(V, x0, 150, epsilon=eps, sync_every=7)
    same((x, F), want)
    assert stats["rollbacks"] == 0 and st.k == kstop


def test_capped_iterations_are_handed_back(refs):
    """A tiny L: the first iteration sits at the cap, the device applies nothing, the host runs the capped step with its
    full evaluation and re-initialisation -- with and without the line search."""
    V, x0 = design("gauss")
    for linesearch in (True, False):
        want = R.fw_div_step(V, 1e-9, x0, 30, 2.0, linesearch=linesearch)
        (x, F, Ls, T), stats, st = device_div(V, x0, 1e-9, 30, 2.0, linesearch=linesearch, sync_every=7)
        same((x, F, Ls), want)
        assert stats["handed_back"] >= 1 and stats["rollbacks"] == 0 and (linesearch or st.reinits >= 1)
        print("linesearch", linesearch, stats, "re-initialisations", st.reinits)


@pytest.mark.parametrize("reason,fields,kw,exc,msg", [
    (SLOPE, dict(slope=2e-6), {}, ValueError, "grad_d_prod must be non-positive"),
    (MIN_X, dict(min_x=0.0), {}, AssertionError, "Entries of x or y not positive."),
    (MIN_X, dict(min_x=math.nan), {}, AssertionError, "Entries of x or y not positive."),
    (L_INF, dict(sum_u2=math.nan), dict(L=1e300, at=0), AssertionError, "L is infinite"),
    (BUDGET, dict(sum_u2=math.nan), dict(ls_ratio=1.2), AssertionError, "L is infinite"),
    (PIVOT, dict(i=1000), {}, ValueError, "accbpg_fw_div_probe_step: bad argument"),
    (ARITH, dict(div=-3.0), dict(gamma=2.5), TypeError, "not supported between"),
    (ARITH, dict(div=5e-324), dict(L=0.5), ZeroDivisionError, "division"),
], ids=lambda v: str(v) if isinstance(v, int) else None)
def test_hand_back_reasons(reason, fields, kw, exc, msg):
    """Every hand-back reason ends as the sequential solver ends, type and message; the record is planted into the
    probe of iteration 9 (a middle record of a chunk; 0 where the run would not get that far), for the device's predictor
    and the host alike."""
    V, x0 = design("gauss")
    args = dict(L=1.0, gamma=2.0, ls_ratio=2, at=9)
    args.update(kw)
    plant = lambda s: s.plant.update({args["at"]: fields})      # noqa: E731
    with pytest.raises(exc) as want:
        sequential_div(V, x0, args["L"], 30, args["gamma"], ls_ratio=args["ls_ratio"], prepare=plant)
    assert msg in str(want.value)
    seen = {}

    def prepare(s):
        plant(s)
        real = s.run_div

        def spy(*a):
            out = real(*a)
            seen.update({(r.status, r.reason): len(out) for r in out if r.status == HANDED_BACK})
            return out
        s.run_div = spy
    with pytest.raises(exc) as got:
        device_div(V, x0, args["L"], 30, args["gamma"], ls_ratio=args["ls_ratio"], sync_every=7, prepare=prepare)
    assert str(got.value) == str(want.value)
    assert seen == {(HANDED_BACK, reason): args["at"] % 7 + 1}  # iteration 9 = the third record of the chunk 7..13
