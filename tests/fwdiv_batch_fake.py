"""Helpers of the CPU tests of the device-predicted Bregman-step batches: a predictor of the decisions of one iteration
as include/accbpg_hip.h states them for the device (accbpg_fw_div_run, written out here apart from the package's text, so
a replay compares two texts), chains of records made with it, and ``FakeBatch``: what the batch-device generators ask of
a DOptimalBatch, answered by one tests/fwdiv_numpy.State per instance.  Like the device, the fake applies what IT
decided, lets an instance that stopped or was handed back idle through the rest of a call, and on request falsifies one
prediction of one instance.  No GPU."""
import math
from types import SimpleNamespace

import numpy as np

import fwdiv_numpy as R

FILL, FLOOR, TRIALS_MAX, RUN_MAX = 1e-15, 1e-6, 64, 1024
LINESEARCH, FIXED_L, CLASSICAL = 0, 1, 2
APPLIED, STOPPED, HANDED_BACK = 0, 1, 2
BUDGET, L_INF, SLOPE, MIN_X, PIVOT, CAP, ARITH = range(1, 8)
END, AGREED_STOP, DEVICE_HB, HOST_HB, DISAGREE, BAD_PIVOT = range(6)
RAISES = (ZeroDivisionError, OverflowError, ValueError, TypeError)
FIELDS = ("i", "w_i", "x_i", "sum_w", "sum_w2", "slope", "div", "min_x", "sum_u2")
STEP_FIELDS = ("L", "a", "hcoef", "hdiv", "ld1", "q1", "f1")


def scalars(a, rec, ld, q, m, radius):
    """(hcoef, hdiv, ld1, q1, f1) as the header states them for the device"""
    tau = a * (radius - FILL) / (1 - a)
    den = 1 + tau * rec.w_i
    hcoef, hdiv = -tau / den, 1 - a
    ld1 = ld + m * math.log(hdiv) + math.log(den)
    q1 = q + a * (FILL - q)
    return hcoef, hdiv, ld1, q1, -ld1 - q1 * ((rec.sum_w + hcoef * rec.sum_u2) / hdiv)


def blank(probe):
    return SimpleNamespace(probe=probe, L=0.0, trials=0, a=0.0, hcoef=0.0, hdiv=0.0, ld1=0.0, q1=0.0, f1=0.0,
                           status=APPLIED, reason=0)


def predict(probe, n, bk, mode, gamma, ls_ratio, eps, k, flip=None):
    """Modes 0 and 1: the record of iteration k from its probe; the book ``bk`` (ld, q, m, radius, F_prev, L) advances
    unless the iteration is handed back."""
    r = blank(probe)
    r.ld1, r.q1 = bk.ld, bk.q

    def back(reason):
        r.status, r.reason = HANDED_BACK, reason
        return r
    fx = -bk.ld - bk.q * probe.sum_w
    if not 0 <= probe.i < n:
        return back(PIVOT)
    div = probe.div if probe.div != 0 else FLOOR
    slope = 0.0 if 0 < probe.slope <= FLOOR else probe.slope
    if slope > 0:
        return back(SLOPE)
    if not probe.min_x > 0:
        return back(MIN_X)
    L = bk.L
    try:
        if mode == LINESEARCH:
            L = L / ls_ratio
        for t in range(TRIALS_MAX):
            root = (-slope / (2 * L * div)) ** (1 / (gamma - 1))
            a = 1.0 if 1.0 < root else root
            if not a < 1:
                return back(CAP)
            if flip == "ulp":
                a = float(np.nextafter(a, 0.0))
            r.trials = t + 1
            hcoef, hdiv, ld1, q1, f1 = scalars(a, probe, bk.ld, bk.q, bk.m, bk.radius)
            r.a, r.hcoef, r.hdiv, r.ld1, r.q1, r.f1 = a, hcoef, hdiv, ld1, q1, f1
            if mode != LINESEARCH:
                break
            if math.isinf(L):
                return back(L_INF)
            accept = f1 <= fx + a * slope + a ** gamma * L * div
            if flip == "accept" and t == 0:
                accept = not accept
            if accept:
                break
            L = L * ls_ratio
        else:
            return back(BUDGET)
    except RAISES:
        return back(ARITH)
    stop = k > 0 and abs(fx - bk.F_prev) < eps
    if flip == "stop":
        stop = not stop
    bk.ld, bk.q, bk.F_prev, bk.L = r.ld1, r.q1, fx, L
    r.L, r.status = L, STOPPED if stop else APPLIED
    return r


def predict_classical(prev, probe, n, bk, eps, k, flip=None):
    """Mode 2: the record of iteration k -- the step from the probe ``prev`` before it, then the stop test on the probe
    ``probe`` behind it (a callable: it is taken after the step); a hand-back applies nothing."""
    a = 2 / (k + 2)
    if flip == "ulp":
        a = float(np.nextafter(a, 0.0))
    try:
        hcoef, hdiv, ld1, q1, _ = scalars(a, prev, bk.ld, bk.q, bk.m, bk.radius)
    except RAISES:
        r = blank(prev)
        r.status, r.reason = HANDED_BACK, ARITH
        return r
    bk.ld, bk.q = ld1, q1
    r = blank(probe(a, hcoef, hdiv))
    r.a, r.hcoef, r.hdiv, r.ld1, r.q1 = a, hcoef, hdiv, ld1, q1
    r.f1 = -bk.ld - bk.q * r.probe.sum_w
    norm = math.sqrt(r.probe.sum_w2) if r.probe.sum_w2 >= 0 else math.nan      # (the device's sqrt raises nothing)
    stop = abs(r.f1 - bk.F_prev) < eps or norm < eps
    bk.F_prev = r.f1
    if flip == "stop":
        stop = not stop
    r.status = STOPPED if stop else APPLIED
    return r


def to_ctypes(recs, lead=None):
    """The records as an array of accbpg_fw_div_step (the package's ctypes mirror); ``lead``: a probe in front of them."""
    from accbpg_and_fw_amd import _lib
    off = 0 if lead is None else 1
    arr = (_lib.FwDivStep * max(1, len(recs) + off))()
    if lead is not None:
        for f in FIELDS:
            setattr(arr[0].probe, f, getattr(lead, f))
    for j, r in enumerate(recs):
        s = arr[off + j]
        for f in FIELDS:
            setattr(s.probe, f, getattr(r.probe, f))
        for f in STEP_FIELDS + ("trials", "status", "reason"):
            setattr(s, f, getattr(r, f))
    return arr


class FakeBatch:
    """What the batch-device generators ask of a DOptimalBatch, on one fwdiv_numpy.State per instance."""

    def __init__(self, Vs):
        self.Vs = [np.ascontiguousarray(V) for V in Vs]
        self.K = len(Vs)
        self.m, self.n = self.Vs[0].shape
        self.states = [None] * self.K
        self.recs = [None] * self.K                             # the pending probe of each instance
        self.saved = [None] * self.K
        self.radius = None
        self.log = []                                           # (call, instances it covered[, nsteps, k0s])
        self.flips = {}                                         # (instance, its iteration) -> "accept" | "ulp" | "stop"
        self.restored = []
        self.inits = [0] * self.K
        self.applied = [0] * self.K                             # rank-one steps of each instance, roll-backs undone

    def _idx(self, active):
        return [i for i in range(self.K) if active is None or active[i]]

    # -- what the lock-step solvers of DESIGN 6g ask
    def fw_rows(self, x0):
        x0 = np.asarray(x0, dtype=np.float64)
        X = np.tile(x0, (self.K, 1)) if x0.ndim == 1 else x0.copy()
        assert X.shape == (self.K, self.n)
        return X, True

    def fw_init(self, X, active=None, named=False):
        idx = self._idx(active)
        self.log.append(("init", tuple(idx)))
        out = [float("nan")] * self.K
        for i in idx:
            try:
                if self.states[i] is None:
                    self.states[i] = R.State(self.Vs[i], X[i])
                else:
                    self.states[i].init(np.array(X[i], dtype=np.float64))
            except ValueError as err:
                raise ValueError(("instance %d: " % i if named else "") + str(err)) from None
            self.recs[i] = None
            self.inits[i] += 1
            out[i] = self.states[i].ld
        return out

    def fw_x(self, i, as_numpy=True):
        return self.states[i].x.copy()

    def _probe(self, i):
        self.recs[i] = self.states[i].probe(self.radius)
        return SimpleNamespace(**{k: self.recs[i][k] for k in FIELDS})

    def fw_div_probe(self, active=None, radius=1):
        idx = self._idx(active)
        self.log.append(("probe", tuple(idx)))
        self.radius = radius
        out = [None] * self.K
        for i in idx:
            out[i] = self._probe(i)
        return out

    def _apply(self, i, p, a, hcoef, hdiv):
        assert self.recs[i] is not None and p == self.recs[i]["i"], "apply without the probe before it"
        self.states[i].apply(self.recs[i], a, self.radius, hcoef, hdiv)
        self.recs[i] = None
        self.applied[i] += 1

    def steps_applied(self, i):
        return self.applied[i]

    def fw_div_apply(self, active, applies):
        idx = self._idx(active)
        self.log.append(("apply", tuple(idx)))
        for i in idx:
            self._apply(i, *applies[i])

    def fw_div_capped(self, i, p, radius, valued):
        self.log.append(("capped", (i,)))
        st = self.states[i]
        s = np.full(self.n, R.FILL)
        s[p] = radius
        trial = st.x + 1.0 * (s - st.x)
        return trial, (R._value(st.V, trial) if valued else None)

    # -- what the device-predicted form adds
    def fw_snapshot(self, active=None):
        idx = self._idx(active)
        self.log.append(("snapshot", tuple(idx)))
        for i in idx:
            st = self.states[i]
            self.saved[i] = (st.x.copy(), st.w.copy(), st.H.copy(), self.applied[i])

    def fw_restore(self, i):
        self.log.append(("restore", (i,)))
        self.restored.append(i)
        st = self.states[i]
        st.x, st.w, st.H = (v.copy() for v in self.saved[i][:3])
        self.applied[i] = self.saved[i][3]
        self.recs[i] = None

    def fw_div_run(self, mode, params, nsteps, active=None, radius=1):
        idx = self._idx(active)
        assert 1 <= nsteps <= RUN_MAX and idx
        self.log.append(("run", tuple(idx), nsteps, tuple(params[i][0] for i in idx)))
        self.radius = radius
        out = [None] * self.K
        for i in idx:
            k0, L, gamma, ls_ratio, eps, ld, q, F_prev = params[i]
            bk = SimpleNamespace(ld=ld, q=q, m=self.m, radius=radius, F_prev=F_prev, L=L)
            rows, flipped = [], False
            if mode == CLASSICAL:
                assert self.recs[i] is not None and k0 >= 1, "accbpg_dopt_batch_fw_div_run: no probe pending"
            for j in range(nsteps):
                k = k0 + j
                # (one per call and instance: what follows a falsified record is thrown away by the host)
                flip = self.flips.pop((i, k), None) if not flipped else None
                flipped = flipped or flip is not None
                if mode == CLASSICAL:
                    prev = SimpleNamespace(**{f: self.recs[i][f] for f in FIELDS})

                    def step_and_probe(a, hcoef, hdiv, i=i, prev=prev):
                        self._apply(i, prev.i, a, hcoef, hdiv)
                        return self._probe(i)
                    r = predict_classical(prev, step_and_probe, self.n, bk, eps, k, flip)
                else:
                    r = predict(self._probe(i), self.n, bk, mode, gamma, ls_ratio, eps, k, flip)
                    if r.status != HANDED_BACK:
                        self._apply(i, r.probe.i, r.a, r.hcoef, r.hdiv)
                rows.append(r)
                if r.status != APPLIED:                         # the instance idles through the rest of the call
                    break
            out[i] = rows
        return out

    def fw_div_replay(self, i, prm, recs, pending=None):
        from accbpg_and_fw_amd import _lib, batched
        return batched._lib_fw_div_replay(_lib.load(), prm, self.n, self.m, FILL, float(self.radius), recs, pending)

    def bad_div_pivot(self, i):
        raise ValueError("instance %d: accbpg_fw_div_probe_step: bad argument (pivot index outside [0, n))" % i)
