"""Frank-Wolfe and Wolfe-Atwood (away-step) solvers for D-optimal design with the
reference's signatures and return tuples (accbpg/D_opt_alg.py:9-88, 91-185).

State (x, the inverse H = (V X V^T)^-1, w_i = v_i^T H v_i) lives on the GPU inside
the D-optimal handle; per iteration the host reads back one small probe record
(argmax / away index and their values), takes the scalar decisions exactly as the
reference writes them, and issues one rank-one update.
"""
from __future__ import annotations

import copy
import ctypes as C
import math
import struct
import time

import numpy as np
import torch

from . import _lib
from .algorithms_fw import _SLOPE_FLOOR, _check_options, _step_length
from .functions import DOptimalObj, _ptr, _stream, from_dev, to_dev, vec_axpby, vec_vertex


class _FWState:
    """Owns the handle-side Frank-Wolfe state for one run."""

    def __init__(self, V, x0):
        self.obj = V if isinstance(V, DOptimalObj) else DOptimalObj(V)
        self.lib = _lib.load()
        self.h = self.obj._h
        self.m, self.n = self.obj.m, self.obj.n
        x0d, self.as_numpy = to_dev(x0)
        logdet = C.c_double(0.0)
        with torch.cuda.device(self.obj.device):
            self.lib.accbpg_dopt_set_stream(self.h, _stream())
            rc = self.lib.accbpg_fw_init(self.h, _ptr(x0d), C.byref(logdet))
        _lib.check(rc, "accbpg_fw_init")
        self.logdet_gram = logdet.value
        self._steps = None

    def _on_device(self):
        """True when the objective's device is already the current one (then the two calls per iteration skip the
        device context manager: a few microseconds each, against a step of 0.12-0.15 ms)."""
        return torch.cuda.current_device() == self.obj.device.index

    def probe(self, away, refresh_logdet):
        pr = _lib.FwProbe()
        if self._on_device():
            rc = self.lib.accbpg_fw_probe_step(self.h, int(away), int(refresh_logdet), C.byref(pr))
        else:
            with torch.cuda.device(self.obj.device):
                rc = self.lib.accbpg_fw_probe_step(self.h, int(away), int(refresh_logdet), C.byref(pr))
        if rc:
            _lib.check(rc, "accbpg_fw_probe_step")
        return pr

    def logdet_ring(self, depth, small_launches=2):
        """How many side factorisations of ``probe(refresh_logdet=2)`` may be in flight, and how they run."""
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_logdet_ring(self.h, int(depth), int(small_launches))
        _lib.check(rc, "accbpg_fw_logdet_ring")

    def flush_logdet(self):
        """log det(H) of the oldest ``probe(refresh_logdet=2)`` call still in flight (see accbpg_fw_logdet_flush)."""
        out = C.c_double(0.0)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_logdet_flush(self.h, C.byref(out))
        _lib.check(rc, "accbpg_fw_logdet_flush")
        return out.value

    def update(self, p, xscale, xadd, hcoef, hdiv):
        if self._on_device():
            rc = self.lib.accbpg_fw_update(self.h, int(p), float(xscale), float(xadd), float(hcoef), float(hdiv))
        else:
            with torch.cuda.device(self.obj.device):
                rc = self.lib.accbpg_fw_update(self.h, int(p), float(xscale), float(xadd), float(hcoef), float(hdiv))
        if rc:
            _lib.check(rc, "accbpg_fw_update")

    def snapshot(self):
        """Start the side factorisation of the current H (accbpg_fw_logdet_snapshot); returns the value that comes in."""
        out = C.c_double(0.0)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_logdet_snapshot(self.h, C.byref(out))
        _lib.check(rc, "accbpg_fw_logdet_snapshot")
        return out.value

    def run(self, away, eps, nsteps):
        """``nsteps`` iterations decided on the device behind one synchronisation (accbpg_fw_run): the records of the
        iterations that ran.  A record with status 2 (pivot outside [0, n)) is returned, not raised: the replay reaches it
        in its turn and calls ``bad_pivot``."""
        if self._steps is None:
            self._steps = (_lib.FwStep * _lib.FW_RUN_MAX)()
        nrun = C.c_int(0)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_run(self.h, int(away), float(eps), int(nsteps), self._steps, C.byref(nrun))
        if rc and not (rc == _lib.ERR_ARG and nrun.value > 0 and self._steps[nrun.value - 1].status == _lib.FW_BAD_PIVOT):
            _lib.check(rc, "accbpg_fw_run")
        return [self._steps[k] for k in range(nrun.value)]

    def bad_pivot(self):
        """The exception of the sequential solver's ``update`` with such a pivot (the library's last error is still the
        message accbpg_fw_run left)."""
        _lib.check(_lib.ERR_ARG, "accbpg_fw_update")

    def x(self):
        out = torch.empty(self.n, dtype=torch.float64, device=self.obj.device)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_get_state(self.h, _ptr(out), None, None)
        _lib.check(rc, "accbpg_fw_get_state")
        return from_dev(out, self.as_numpy)

    def state(self):
        x = torch.empty(self.n, dtype=torch.float64, device=self.obj.device)
        w = torch.empty(self.n, dtype=torch.float64, device=self.obj.device)
        H = torch.empty(self.m, self.m, dtype=torch.float64, device=self.obj.device)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_get_state(self.h, _ptr(x), _ptr(w), _ptr(H))
        _lib.check(rc, "accbpg_fw_get_state")
        return x, w, H


def _drain(gen):
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def _fw_decide(m, w_i, w_j, eps):
    """The scalar decisions of one Frank-Wolfe iteration, as the reference writes them (D_opt_alg.py:63-64, :72,
    :75-80), from the probe's w_i = max w and w_j = min of w over the support.  Returns (eps_pos, eps_neg, update,
    detmul): update = (xscale, xadd, hcoef, hdiv) of the rank-one update with pivot i, or None when the stop test
    holds; detmul the factor det(V X V^T) takes (:80).  One copy for the single and the lock-step solver."""
    eps_pos = w_i / m - 1                                       # :63
    eps_neg = 1 - w_j / m                                       # :64
    if eps_pos <= eps and eps_neg <= eps:                       # :72
        return eps_pos, eps_neg, None, None
    t = (w_i / m - 1) / (w_i - 1)                               # :75
    coef = t / (1 + t * (w_i - 1))                              # :79,:82
    detmul = np.power(1 - t, m - 1) * (1 + t * (w_i - 1))       # :80
    return eps_pos, eps_neg, (1 - t, t, -coef, 1 - t), detmul   # :76-79,:82


def D_opt_FW(V, x0, eps, maxitrs, verbose=True, verbskip=1):
    """Frank-Wolfe with exact line search (accbpg/D_opt_alg.py:9-88).
    Returns (x, F, SP, SN, T).  F[k] = -log(detVXVT) with the determinant tracked by
    the rank-one formula (:52,:80); w is never refreshed; the stop test precedes the
    update so x matches F[-1] (:72).  ``V`` may be a matrix or a DOptimalObj."""
    return _drain(D_opt_FW_steps(V, x0, eps, maxitrs, verbose, verbskip))


def D_opt_FW_steps(V, x0, eps, maxitrs, verbose=True, verbskip=1):
    """Generator form of D_opt_FW: yields k after each update, returns D_opt_FW's tuple."""
    start_time = time.time()
    st = _FWState(V, x0)
    m = st.m
    F = np.zeros(maxitrs)
    SP = np.zeros(maxitrs)
    SN = np.zeros(maxitrs)
    T = np.zeros(maxitrs)
    detVXVT = np.exp(st.logdet_gram)                            # :41

    if verbose:
        print("\nSolving D-opt design problem using Frank-Wolfe method")
        print("     k      F(x)     pos_slack   neg_slack    time")

    k = -1
    for k in range(maxitrs):
        F[k] = - np.log(detVXVT)                                # :52
        T[k] = time.time() - start_time
        pr = st.probe(away=0, refresh_logdet=0)                 # :59-61
        eps_pos, eps_neg, upd, detmul = _fw_decide(m, pr.w_i, pr.w_j, eps)
        SP[k] = eps_pos
        SN[k] = eps_neg

        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:6.1f}".format(
                k, F[k], eps_pos, eps_neg, T[k]))

        if upd is None:                                         # :72
            break

        st.update(pr.i, *upd)                                   # :76-79,:82
        detVXVT *= detmul                                       # :80
        yield k

    return st.x(), F[0:k + 1], SP[0:k + 1], SN[0:k + 1], T[0:k + 1]


# How often D_opt_FW_away refactors the maintained inverse for F[k] = log det(H_k) when the caller does not say
# (``logdet_refresh=None``), and how many factorisations are in flight when it does so every iteration.  Decided with
# numbers (tools/fw_away_modes.py, profiles/r03_fw_away_modes.json; D_opt_design(2048,32768), one MI355X): anchoring
# every 16th iteration leaves F[k] within 1.1e-13 (absolute; |F| ~ 50) of the every-iteration factorisation over 1000
# and over 20000 iterations -- less than that run's own distance from the reference's trace (1e-14 relative) -- with
# bit-identical iterates and gaps, at 5600-5900 iterations/s against 2800-2900 for the every-iteration form with three
# factorisations in flight (1520 with one).  The every-iteration form stays one keyword away (logdet_refresh=1).
LOGDET_REFRESH_DEFAULT = 16
LOGDET_RING_DEFAULT = 3


def _away_modes(logdet_refresh, logdet_ring):
    """(R, depth) of D_opt_FW_away's ``logdet_refresh`` / ``logdet_ring`` keywords."""
    R = LOGDET_REFRESH_DEFAULT if logdet_refresh is None else int(logdet_refresh)
    depth = LOGDET_RING_DEFAULT if logdet_ring is None else int(logdet_ring)
    if R != 1:
        depth = 1                                               # anchors are R iterations apart: one in flight is enough
    return R, depth


class _AwayRun:
    """Host side of ONE away-step run: the traces, the bookkeeping of F[k] = log det(H_k) (anchors in flight, log-space
    steps between them) and the scalar decisions of an iteration as the reference writes them (D_opt_alg.py:150-179).
    One copy for the single and the lock-step solver.

    F[k] is filled in (and its table row printed) when its value is in: an anchor -- a fresh factorisation of H_a
    started at iteration a on a side stream -- arrives `depth` refreshing iterations later; the iterations between
    two anchors follow from the first by the log-space steps, each known one probe after its update (q_prev)."""

    def __init__(self, m, maxitrs, R, depth, verbose=False, verbskip=1):
        self.m, self.R, self.depth = m, R, depth
        self.verbose, self.verbskip = verbose, verbskip
        self.F = np.zeros(maxitrs)
        self.SP = np.zeros(maxitrs)
        self.SN = np.zeros(maxitrs)
        self.T = np.zeros(maxitrs)
        self.anchors = []            # iterations whose factorisation is in flight, oldest first
        self.delta = np.zeros(maxitrs)   # delta[k] = log det(H_{k+1}) - log det(H_k) by the determinant lemma
        self.filled = 0              # F[0:filled] is final
        self.step = None             # (hcoef, hdiv) of the update applied at the previous iteration
        self.k = -1                  # last iteration that ran

    def refresh(self, k):
        """Does iteration k start a factorisation of H_k?"""
        return (self.R > 0) and (k % self.R == 0)

    def fill(self, upto):
        """F[filled:upto] from F[filled-1] by the log-space steps (upto exclusive), and print their rows."""
        for j in range(self.filled, upto):
            self.F[j] = self.F[j - 1] + self.delta[j - 1]
            self.row(j)
        self.filled = max(self.filled, upto)

    def row(self, j):
        if self.verbose and j % self.verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:6.1f}".format(j, self.F[j], self.SP[j], self.SN[j],
                                                                             self.T[j]))

    def settle(self, a, value):
        """The anchor of iteration a is in."""
        self.fill(a)
        self.F[a] = value
        self.row(a)
        self.filled = a + 1

    def iterate(self, k, pr, collected, now, logdet_gram, eps):
        """Iteration k from its probe record `pr`; `collected`: the anchor value that came in with this iteration's
        snapshot (refreshing iterations only).  Returns (p, xscale, xadd, hcoef, hdiv) of the update, or None when the
        stop test holds."""
        m = self.m
        self.k = k
        self.T[k] = now
        if self.step is not None:
            hcoef, hdiv = self.step
            arg = hcoef * pr.q_prev
            self.delta[k - 1] = (math.log1p(arg) - m * math.log(hdiv)) if (arg > -1.0 and hdiv > 0.0) else float("nan")
        if self.refresh(k):
            if len(self.anchors) >= self.depth:
                self.settle(self.anchors.pop(0), collected)
            self.anchors.append(k)
        elif self.R == 0 and k == 0:
            self.F[0] = -logdet_gram
            self.filled = 1
        w_i, w_j = pr.w_i, pr.w_j
        eps_pos = w_i / m - 1                                   # :150
        eps_neg = 1 - w_j / m                                   # :151
        self.SP[k] = eps_pos
        self.SN[k] = eps_neg
        if self.R == 0 and k == 0:
            self.row(0)

        if eps_pos <= eps and eps_neg <= eps:                   # :159
            return None

        if eps_pos >= eps_neg:                                  # :162-170
            t = (w_i / m - 1) / (w_i - 1)
            coef = t / (1 - t + t * w_i)
            self.step = (-coef, 1 - t)
            return (pr.i, 1 - t, t, -coef, 1 - t)
        x_j = pr.x_j                                            # :171-179
        t = min((1 - w_j / m) / (w_j - 1), x_j / (1 - x_j))
        coef = t / (1 + t - t * w_j)
        self.step = (coef, 1 + t)
        return (pr.j, 1 + t, -t, coef, 1 + t)

    def finish(self, flush):
        """Collect the anchors still in flight (`flush()` returns the oldest) and fill F to the end; returns
        (F, SP, SN, T) cut to the iterations that ran."""
        while self.anchors:
            self.settle(self.anchors.pop(0), flush())
        self.fill(self.k + 1)
        e = self.k + 1
        return self.F[0:e], self.SP[0:e], self.SN[0:e], self.T[0:e]


def D_opt_FW_away(V, x0, eps, maxitrs, verbose=True, verbskip=1, logdet_refresh=None, logdet_ring=None):
    """Frank-Wolfe with Wolfe's away steps (accbpg/D_opt_alg.py:91-185).
    Returns (x, F, SP, SN, T).  F[k] = log det(H_k) of the maintained inverse (:136), a logged value that no decision
    of the iteration reads; iterates, gaps and step choices do not depend on how it is formed.

    ``logdet_refresh`` (extension): 1 = the reference's computation, a fresh factorisation of H_k for every k (formed
    beside the steps, ``logdet_ring`` of them in flight, F[k] filled in that many iterations late).  R > 1 = a fresh
    factorisation of H_k for every k that is a multiple of R (beside the steps as well); in between log det(H) is
    advanced in log space by the matrix determinant lemma for the very rank-one update the step applies,
    log det(H+) = log det(H) + log(1 + c q) - m log(d) with q = v^T H v of the pivot column in the inverse as
    maintained (computed on the device from H itself, not the tracked w), so the error of F[k] against a fresh
    factorisation is the rounding of at most R - 1 such terms.  0 = never refactor (lemma from the start).
    None = ``LOGDET_REFRESH_DEFAULT``."""
    return _drain(D_opt_FW_away_steps(V, x0, eps, maxitrs, verbose, verbskip, logdet_refresh, logdet_ring))


def D_opt_FW_away_steps(V, x0, eps, maxitrs, verbose=True, verbskip=1, logdet_refresh=None, logdet_ring=None):
    """Generator form of D_opt_FW_away: yields k after each update, returns D_opt_FW_away's tuple."""
    start_time = time.time()
    st = _FWState(V, x0)
    R, depth = _away_modes(logdet_refresh, logdet_ring)
    st.logdet_ring(depth)
    run = _AwayRun(st.m, maxitrs, R, depth, verbose, verbskip)

    if verbose:
        print("\nSolving D-opt design problem using Frank-Wolfe method with away steps")
        print("     k      F(x)     pos_slack   neg_slack    time")

    for k in range(maxitrs):
        pr = st.probe(away=1, refresh_logdet=2 if run.refresh(k) else 0)   # :136, :145-147
        upd = run.iterate(k, pr, pr.logdet_H, time.time() - start_time, st.logdet_gram, eps)
        if upd is None:                                         # :159
            break
        st.update(*upd)
        yield k

    F, SP, SN, T = run.finish(st.flush_logdet)
    return st.x(), F, SP, SN, T


# ---- several iterations per host round trip ----------------------------------------------------------------------------
SYNC_EVERY_DEFAULT = 64
_GUARD_FIELDS = ("p", "xscale", "xadd", "hcoef", "hdiv")


def _guard(st, k, rec, upd):
    """The device's decision of iteration k (record ``rec`` of accbpg_fw_run) against the host's own ``upd`` -- (p,
    xscale, xadd, hcoef, hdiv), or None when the stop test holds -- bit for bit (a NaN equals a NaN).  Raises RuntimeError naming k and the
    field; a pivot outside [0, n) raises what the sequential solver's update raises."""
    if upd is None:
        if rec.status != _lib.FW_STOPPED:
            raise RuntimeError("iteration %d: the host's stop test holds, the device's did not (field status = %d)"
                               % (k, rec.status))
        return
    if rec.status == _lib.FW_STOPPED:
        raise RuntimeError("iteration %d: the device's stop test held, the host's does not (field status = 1)" % k)
    for name, mine, fmt in zip(_GUARD_FIELDS, upd, "qdddd"):
        theirs = getattr(rec, name)
        if struct.pack(fmt, mine) != struct.pack(fmt, theirs) and not (mine != mine and theirs != theirs):   # (NaN for NaN)
            raise RuntimeError("iteration %d: field %s decided on the device (%r) differs from the host's (%r)"
                               % (k, name, theirs, mine))
    if rec.status == _lib.FW_BAD_PIVOT:
        st.bad_pivot()
    if rec.status != _lib.FW_APPLIED:
        raise RuntimeError("iteration %d: unexpected field status = %d" % (k, rec.status))


def _chunk(k, maxitrs, sync_every, R=0):
    """Iterations of the chunk that starts at k: ``sync_every`` (None: R, or SYNC_EVERY_DEFAULT when R = 0), cut so
    that the chunk ends before the next multiple of R (R > 0), at maxitrs, and at what one call holds."""
    S = (R if R > 0 else SYNC_EVERY_DEFAULT) if sync_every is None else int(sync_every)
    if S < 1:
        raise ValueError("sync_every must be at least 1")
    if R > 0:
        S = min(S, R - k % R)
    return min(S, maxitrs - k, _lib.FW_RUN_MAX)


def D_opt_FW_device(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=SYNC_EVERY_DEFAULT):
    """D_opt_FW with ``sync_every`` iterations per host round trip; T[k] of all iterations of a chunk is the time at
    which the chunk's records arrived, and the table rows are printed per chunk, in order k = 0, 1, 2, ...

    The stop test, the step length and the rank-one coefficients of an iteration are computed on the device
    (accbpg_fw_run) by the sequential solver's kernels on its grids; the host replays every record through
    ``_fw_decide`` for F, SP and SN and compares its own update scalars with the device's bit for bit (RuntimeError on
    a difference).  Returns D_opt_FW's tuple; x, F, SP, SN and the iteration count are bit-identical to D_opt_FW's."""
    return _drain(D_opt_FW_device_steps(V, x0, eps, maxitrs, verbose, verbskip, sync_every))


def D_opt_FW_device_steps(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=SYNC_EVERY_DEFAULT):
    """Generator form of D_opt_FW_device: yields the last k of each chunk, returns D_opt_FW_device's tuple."""
    return _fw_device_steps(_FWState(V, x0), eps, maxitrs, verbose, verbskip, sync_every, time.time())


def _fw_device_steps(st, eps, maxitrs, verbose, verbskip, sync_every, start_time):
    """D_opt_FW_device_steps on a state object (``m``, ``logdet_gram``, ``run``, ``bad_pivot``, ``x``)."""
    m = st.m
    F = np.zeros(maxitrs)
    SP = np.zeros(maxitrs)
    SN = np.zeros(maxitrs)
    T = np.zeros(maxitrs)
    detVXVT = np.exp(st.logdet_gram)                            # :41

    if verbose:
        print("\nSolving D-opt design problem using Frank-Wolfe method")
        print("     k      F(x)     pos_slack   neg_slack    time")

    k = -1
    stopped = False
    while k + 1 < maxitrs and not stopped:
        recs = st.run(0, eps, _chunk(k + 1, maxitrs, sync_every))
        now = time.time() - start_time
        for rec in recs:
            k += 1
            F[k] = - np.log(detVXVT)                            # :52
            T[k] = now
            eps_pos, eps_neg, upd, detmul = _fw_decide(m, rec.w_i, rec.w_j, eps)
            SP[k] = eps_pos
            SN[k] = eps_neg
            if verbose and k % verbskip == 0:
                print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:6.1f}".format(
                    k, F[k], eps_pos, eps_neg, T[k]))
            _guard(st, k, rec, None if upd is None else (rec.i,) + upd)
            if upd is None:                                     # :72
                stopped = True
                break
            detVXVT *= detmul                                   # :80
        if not stopped:
            yield k

    return st.x(), F[0:k + 1], SP[0:k + 1], SN[0:k + 1], T[0:k + 1]


def D_opt_FW_away_device(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=None, logdet_refresh=None,
                         logdet_ring=None):
    """D_opt_FW_away with up to ``sync_every`` iterations per host round trip; T[k] of all iterations of a chunk is the
    time at which the chunk's records arrived, and the table rows are printed per chunk, in order k = 0, 1, 2, ...

    The stop test, the choice between a Frank-Wolfe and an away step, the step length and the rank-one coefficients are
    computed on the device (accbpg_fw_run); the host replays every record through ``_AwayRun.iterate`` and compares
    its own update scalars with the device's bit for bit (RuntimeError on a difference).  A chunk never spans an
    iteration that refactors H (a multiple of R = ``logdet_refresh``): it ends before the next one, the snapshot is
    issued between chunks, and F is formed as D_opt_FW_away forms it.  ``sync_every=None`` means R (64 when R = 0);
    R = 1 gives chunks of one.  Returns D_opt_FW_away's tuple, x, F, SP, SN and the iteration count bit-identical to it
    for the same ``logdet_refresh`` / ``logdet_ring``."""
    return _drain(D_opt_FW_away_device_steps(V, x0, eps, maxitrs, verbose, verbskip, sync_every, logdet_refresh,
                                             logdet_ring))


def D_opt_FW_away_device_steps(V, x0, eps, maxitrs, verbose=True, verbskip=1, sync_every=None, logdet_refresh=None,
                               logdet_ring=None):
    """Generator form of D_opt_FW_away_device: yields the last k of each chunk, returns its tuple."""
    return _away_device_steps(_FWState(V, x0), eps, maxitrs, verbose, verbskip, sync_every, logdet_refresh, logdet_ring,
                              time.time())


def _away_device_steps(st, eps, maxitrs, verbose, verbskip, sync_every, logdet_refresh, logdet_ring, start_time):
    """D_opt_FW_away_device_steps on a state object (as _fw_device_steps, and ``logdet_ring``, ``snapshot``,
    ``flush_logdet``)."""
    R, depth = _away_modes(logdet_refresh, logdet_ring)
    st.logdet_ring(depth)
    run = _AwayRun(st.m, maxitrs, R, depth, verbose, verbskip)
    nan = float("nan")

    if verbose:
        print("\nSolving D-opt design problem using Frank-Wolfe method with away steps")
        print("     k      F(x)     pos_slack   neg_slack    time")

    k = 0
    stopped = False
    while k < maxitrs and not stopped:
        collected = st.snapshot() if run.refresh(k) else nan     # :136: the chunk starts on the anchor, or holds none
        recs = st.run(1, eps, _chunk(k, maxitrs, sync_every, R))     # :145-147, :150-179
        now = time.time() - start_time
        for rec in recs:
            upd = run.iterate(k, rec, collected, now, st.logdet_gram, eps)
            collected = nan
            _guard(st, k, rec, upd)
            if upd is None:                                     # :159
                stopped = True
                break
            k += 1
        if not stopped:
            yield k - 1

    F, SP, SN, T = run.finish(st.flush_logdet)
    return st.x(), F, SP, SN, T


# ---- lock-step batches -----------------------------------------------------------------------------------------------
def _batch_x0(batch, x0):
    """x0 (one vector or K x n) as a K x n device tensor with row stride n."""
    x0d, as_numpy = to_dev(x0)
    X = x0d.reshape(1, -1).repeat(batch.K, 1) if x0d.dim() == 1 else x0d.clone()
    X = X.to(batch.device).contiguous()
    assert X.shape == (batch.K, batch.n), "x0: one vector of length n, or a K x n array"
    return X, as_numpy


def _batch_eps(batch, eps):
    """eps (a scalar, or one per instance) as a list of K floats."""
    return [float(v) for v in np.broadcast_to(np.asarray(eps, dtype=np.float64), (batch.K,))]


def D_opt_FW_batch(batch, x0, eps, maxitrs):
    """D_opt_FW on the K instances of a ``DOptimalBatch`` in lock-step: every step kernel is launched once for the
    instances that are still running, and one synchronisation returns all their probe records.  ``x0``: one vector
    or a K x n array; ``eps``: a scalar or one per instance.  The decisions (stop test, step length, tracked
    determinant) are kept per instance exactly as the sequential solver takes them; an instance that meets its stop
    test drops out of the later launches.  Silent.  Returns a list of K tuples (x, F, SP, SN, T), x, F, SP and SN
    bit-identical to ``D_opt_FW(batch.instance(i), x0_i, eps_i, maxitrs, verbose=False)``.

    For a rank's share of many instances (``solve_instances`` hands a solver one problem at a time): build the batch
    from the matrices of ``sharded.split_instances(N, world, rank)`` and call this on it."""
    return _drain(D_opt_FW_batch_steps(batch, x0, eps, maxitrs))


def D_opt_FW_batch_steps(batch, x0, eps, maxitrs):
    """Generator form of D_opt_FW_batch: yields k after each lock-step update, returns D_opt_FW_batch's list."""
    start_time = time.time()
    K, m = batch.K, batch.m
    X0, as_numpy = _batch_x0(batch, x0)
    epsv = _batch_eps(batch, eps)
    logdet = batch.fw_init(X0)
    F = np.zeros((K, maxitrs)); SP = np.zeros((K, maxitrs)); SN = np.zeros((K, maxitrs)); T = np.zeros((K, maxitrs))
    detVXVT = [np.exp(ld) for ld in logdet]                     # :41
    active = [True] * K
    last = [-1] * K
    upd = [None] * K
    for k in range(maxitrs):
        if not any(active):
            break
        now = time.time() - start_time
        for i in range(K):
            if active[i]:
                F[i, k] = - np.log(detVXVT[i])                  # :52
                T[i, k] = now
        prs = batch.fw_probe(0, active)                         # :59-61
        for i in range(K):
            if not active[i]:
                continue
            SP[i, k], SN[i, k], u, detmul = _fw_decide(m, prs[i].w_i, prs[i].w_j, epsv[i])
            last[i] = k
            if u is None:                                       # :72
                active[i] = False
                continue
            upd[i] = (prs[i].i,) + u
            detVXVT[i] *= detmul                                # :80
        if not any(active):
            break
        batch.fw_update(active, upd)                            # :76-79,:82
        yield k
    out = []
    for i in range(K):
        e = last[i] + 1
        out.append((batch.fw_x(i, as_numpy), F[i, :e].copy(), SP[i, :e].copy(), SN[i, :e].copy(), T[i, :e].copy()))
    return out


def D_opt_FW_away_batch(batch, x0, eps, maxitrs, logdet_refresh=None, logdet_ring=None):
    """D_opt_FW_away on the K instances of a ``DOptimalBatch`` in lock-step (see ``D_opt_FW_batch``).  F[k] =
    log det(H_k) is formed per instance as the sequential solver forms it -- ``logdet_refresh`` / ``logdet_ring`` as
    there, each instance's side factorisations on its own handle's ring -- so F, too, is bit-identical to
    ``D_opt_FW_away(batch.instance(i), x0_i, eps_i, maxitrs, verbose=False, logdet_refresh=..., logdet_ring=...)``."""
    return _drain(D_opt_FW_away_batch_steps(batch, x0, eps, maxitrs, logdet_refresh, logdet_ring))


def D_opt_FW_away_batch_steps(batch, x0, eps, maxitrs, logdet_refresh=None, logdet_ring=None):
    """Generator form of D_opt_FW_away_batch: yields k after each lock-step update, returns its list."""
    start_time = time.time()
    K, m = batch.K, batch.m
    X0, as_numpy = _batch_x0(batch, x0)
    epsv = _batch_eps(batch, eps)
    R, depth = _away_modes(logdet_refresh, logdet_ring)
    logdet = batch.fw_init(X0)
    batch.fw_logdet_ring(depth)
    runs = [_AwayRun(m, maxitrs, R, depth) for _ in range(K)]
    active = [True] * K
    upd = [None] * K
    nan = float("nan")
    for k in range(maxitrs):
        if not any(active):
            break
        # anchors: a snapshot of H_k per running instance, each factored beside the steps on its own handle's ring
        collected = batch.fw_logdet_snapshot(active) if runs[0].refresh(k) else [nan] * K      # :136
        prs = batch.fw_probe(1, active)                         # :145-147
        now = time.time() - start_time
        for i in range(K):
            if not active[i]:
                continue
            upd[i] = runs[i].iterate(k, prs[i], collected[i], now, logdet[i], epsv[i])
            if upd[i] is None:                                  # :159
                active[i] = False
        if not any(active):
            break
        batch.fw_update(active, upd)
        yield k
    out = []
    for i in range(K):
        F, SP, SN, T = runs[i].finish(lambda i=i: batch.fw_logdet_flush(i))
        out.append((batch.fw_x(i, as_numpy), F.copy(), SP.copy(), SN.copy(), T.copy()))
    return out


# ---- lock-step batches that decide their steps on the device ---------------------------------------------------------
def _guard_instance(batch, i, k, rec, upd):
    """``_guard`` for instance i of a batch: a difference raises RuntimeError naming the instance as well as k and the
    field; a pivot outside [0, n) raises what the sequential solver's update raises, the instance and k in front."""
    try:
        _guard(batch, k, rec, upd)
    except (RuntimeError, ValueError) as err:
        prefix = "instance %d: " % i if isinstance(err, RuntimeError) else "instance %d, iteration %d: " % (i, k)
        raise type(err)(prefix + str(err)) from None


def D_opt_FW_batch_device(batch, x0, eps, maxitrs, sync_every=SYNC_EVERY_DEFAULT):
    """D_opt_FW_batch with ``sync_every`` iterations per host round trip: the K instances of a ``DOptimalBatch`` share
    every launch, and the stop test, the step length and the rank-one coefficients of every instance are computed on
    the device (accbpg_dopt_batch_fw_run), as D_opt_FW_device computes them for one.  ``x0`` and ``eps`` as
    D_opt_FW_batch takes them.  The host replays every instance's records through ``_fw_decide`` and compares its own
    update scalars with the device's bit for bit (RuntimeError naming the instance, k and the field on a difference).
    An instance that stops inside a chunk idles through the rest of it and is dropped from the next one.  T[k] of all
    iterations of a chunk is the time at which the chunk's records arrived.  Silent.  Returns a list of K tuples
    (x, F, SP, SN, T), x, F, SP, SN and the iteration count bit-identical to
    ``D_opt_FW(batch.instance(i), x0_i, eps_i, maxitrs, verbose=False)``."""
    return _drain(D_opt_FW_batch_device_steps(batch, x0, eps, maxitrs, sync_every))


def D_opt_FW_batch_device_steps(batch, x0, eps, maxitrs, sync_every=SYNC_EVERY_DEFAULT):
    """Generator form of D_opt_FW_batch_device: yields the last k of each chunk, returns its list."""
    start_time = time.time()
    X0, as_numpy = _batch_x0(batch, x0)
    epsv = _batch_eps(batch, eps)
    logdet = batch.fw_init(X0)
    return _fw_batch_device_steps(batch, logdet, epsv, maxitrs, sync_every, start_time, as_numpy)


def _fw_batch_device_steps(batch, logdet, epsv, maxitrs, sync_every, start_time, as_numpy=True):
    """D_opt_FW_batch_device_steps on an initialised batch object (``K``, ``m``, ``fw_run``, ``bad_pivot``, ``fw_x``)."""
    K, m = batch.K, batch.m
    F = np.zeros((K, maxitrs)); SP = np.zeros((K, maxitrs)); SN = np.zeros((K, maxitrs)); T = np.zeros((K, maxitrs))
    detVXVT = [np.exp(ld) for ld in logdet]                     # :41
    active = [True] * K
    last = [-1] * K
    k = 0                                                       # first iteration of the chunk: the running instances share it
    while k < maxitrs and any(active):
        S = _chunk(k, maxitrs, sync_every)
        recs = batch.fw_run(0, epsv, S, active)
        now = time.time() - start_time
        for i in range(K):
            if not active[i]:
                continue
            kk = k
            for rec in recs[i]:
                F[i, kk] = - np.log(detVXVT[i])                 # :52
                T[i, kk] = now
                SP[i, kk], SN[i, kk], upd, detmul = _fw_decide(m, rec.w_i, rec.w_j, epsv[i])
                last[i] = kk
                _guard_instance(batch, i, kk, rec, None if upd is None else (rec.i,) + upd)
                if upd is None:                                 # :72
                    active[i] = False
                    break
                detVXVT[i] *= detmul                            # :80
                kk += 1
        k += S
        if any(active):
            yield k - 1
    out = []
    for i in range(K):
        e = last[i] + 1
        out.append((batch.fw_x(i, as_numpy), F[i, :e].copy(), SP[i, :e].copy(), SN[i, :e].copy(), T[i, :e].copy()))
    return out


def D_opt_FW_away_batch_device(batch, x0, eps, maxitrs, sync_every=None, logdet_refresh=None, logdet_ring=None):
    """D_opt_FW_away_batch with up to ``sync_every`` iterations per host round trip (see D_opt_FW_batch_device and
    D_opt_FW_away_device).  The chunks are cut as D_opt_FW_away_device cuts them -- all running instances share k, a
    chunk never spans a multiple of R = ``logdet_refresh`` -- and the snapshots of the running instances are issued
    between chunks exactly where D_opt_FW_away_batch issues them, so F is formed by the same code from the same
    anchors.  Returns a list of K tuples (x, F, SP, SN, T), x, F, SP, SN and the iteration count bit-identical to
    ``D_opt_FW_away(batch.instance(i), x0_i, eps_i, maxitrs, verbose=False, logdet_refresh=..., logdet_ring=...)``."""
    return _drain(D_opt_FW_away_batch_device_steps(batch, x0, eps, maxitrs, sync_every, logdet_refresh, logdet_ring))


def D_opt_FW_away_batch_device_steps(batch, x0, eps, maxitrs, sync_every=None, logdet_refresh=None, logdet_ring=None):
    """Generator form of D_opt_FW_away_batch_device: yields the last k of each chunk, returns its list."""
    start_time = time.time()
    X0, as_numpy = _batch_x0(batch, x0)
    epsv = _batch_eps(batch, eps)
    logdet = batch.fw_init(X0)
    return _away_batch_device_steps(batch, logdet, epsv, maxitrs, sync_every, logdet_refresh, logdet_ring, start_time,
                                    as_numpy)


def _away_batch_device_steps(batch, logdet, epsv, maxitrs, sync_every, logdet_refresh, logdet_ring, start_time,
                             as_numpy=True):
    """D_opt_FW_away_batch_device_steps on an initialised batch object (as _fw_batch_device_steps, and
    ``fw_logdet_ring``, ``fw_logdet_snapshot``, ``fw_logdet_flush``)."""
    K, m = batch.K, batch.m
    R, depth = _away_modes(logdet_refresh, logdet_ring)
    batch.fw_logdet_ring(depth)
    runs = [_AwayRun(m, maxitrs, R, depth) for _ in range(K)]
    active = [True] * K
    nan = float("nan")
    k = 0
    while k < maxitrs and any(active):
        # anchors: a snapshot of H_k per running instance (:136); the chunk starts on the anchor, or holds none
        collected = batch.fw_logdet_snapshot(active) if runs[0].refresh(k) else [nan] * K
        S = _chunk(k, maxitrs, sync_every, R)
        recs = batch.fw_run(1, epsv, S, active)                 # :145-147, :150-179
        now = time.time() - start_time
        for i in range(K):
            if not active[i]:
                continue
            kk, coll = k, collected[i]
            for rec in recs[i]:
                upd = runs[i].iterate(kk, rec, coll, now, logdet[i], epsv[i])
                coll = nan
                _guard_instance(batch, i, kk, rec, upd)
                if upd is None:                                 # :159
                    active[i] = False
                    break
                kk += 1
        k += S
        if any(active):
            yield k - 1
    out = []
    for i in range(K):
        F, SP, SN, T = runs[i].finish(lambda i=i: batch.fw_logdet_flush(i))
        out.append((batch.fw_x(i, as_numpy), F.copy(), SP.copy(), SN.copy(), T.copy()))
    return out


# ---- Frank-Wolfe with a Bregman step on the maintained state ------------------------------------------
# FW_alg_div_step / FW_alg_descent_step (algorithms_fw.py) on the D-optimal objective with the Burg kernel and the
# simplex LMO, without an O(m^2 n) evaluation per iteration or per line-search trial: the gradient is -w, the step
# x+ = x + a (s - x) towards s = fill + (radius - fill) e_i is a scaling plus a rank-one change of the Gram matrix, and
# every trial value follows from the matrix determinant lemma in host scalars.
_LMO_FILL = 1e-15       # lmo_simplex's entry away from the vertex (functions_lmo.py)
REFRESH_DEFAULT = 256   # steps between two re-initialisations of (H, w, log det) from x


class _DivBook:
    """What the Bregman-step solvers keep beside one instance's Frank-Wolfe state, in host scalars: ``ld`` the log det
    of the tracked Gram matrix, ``q`` the floor mass not in it, ``since`` the steps since the last initialisation.
    Touches no device: the single and the lock-step solvers keep one per instance."""

    def __init__(self, m, radius, refresh, logdet):
        self.m = m
        self.radius = float(radius)
        self.refresh = int(refresh)
        self.reset(logdet)

    def reset(self, logdet):
        """(H, w, log det) were recomputed from x."""
        self.ld, self.q, self.since = logdet, 0.0, 0

    def refresh_due(self):
        return bool(self.refresh) and self.since == self.refresh

    def value(self, rec):
        """f(x) = -log det(V X V^T): the tracked part, and the dense floor term q V V^T to first order (tr(H V V^T) =
        sum w)."""
        return -self.ld - self.q * rec.sum_w

    def scalars(self, a, rec):
        """(hcoef, hdiv, ld1, q1, f1) of a step of length a < 1 towards the vertex of ``rec``."""
        fill = _LMO_FILL
        tau = a * (self.radius - fill) / (1 - a)
        den = 1 + tau * rec.w_i
        hcoef = -tau / den
        hdiv = 1 - a
        ld1 = self.ld + self.m * math.log(hdiv) + math.log(den)
        q1 = self.q + a * (fill - self.q)
        sw1 = (rec.sum_w + hcoef * rec.sum_u2) / hdiv
        f1 = -ld1 - q1 * sw1
        return hcoef, hdiv, ld1, q1, f1

    def stepped(self, ld1, q1):
        """A rank-one step with these scalars was applied."""
        self.ld, self.q = ld1, q1
        self.since += 1


class _DivStepRun:
    """The host side of one instance of D_opt_FW_div_step: from a probe record to what to do next.  One copy for the
    single and the lock-step solver (as ``_fw_decide`` and ``_AwayRun`` are for theirs)."""

    def __init__(self, book, L, maxitrs, gamma, epsilon, linesearch, ls_ratio):
        self.book = book
        self.L, self.gamma, self.epsilon, self.linesearch, self.ls_ratio = L, gamma, epsilon, linesearch, ls_ratio
        self.F = np.zeros(maxitrs)
        self.Ls = np.zeros(maxitrs)
        self.T = np.zeros(maxitrs)
        self.done = 0

    def decide(self, k, rec, now, capped):
        """Iteration k from its probe record.  ``capped(rec)`` builds the trial of the capped step a == 1 and returns
        (trial, f(trial)) -- a full evaluation, as the generic solver's; f is not read without the line search -- and is
        called once per trial at the cap.  Returns (step, trial, stop): step = (p, a, hcoef, hdiv) of the rank-one step
        to apply (the book is advanced here) and trial None, or step None and the trial to re-initialise from (then
        ``book.reset``); stop: the stop test holds, this step is the last."""
        book, linesearch, gamma = self.book, self.linesearch, self.gamma
        fx = book.value(rec)
        self.F[k] = fx
        self.T[k] = now

        div = rec.div if rec.div != 0 else _SLOPE_FLOOR
        slope = rec.slope
        if 0 < slope <= _SLOPE_FLOOR:
            slope = 0.0
        if slope > 0:
            raise ValueError("grad_d_prod must be non-positive")
        assert rec.min_x > 0, "Entries of x or y not positive."

        L = self.L
        if linesearch:
            L = L / self.ls_ratio
        while True:
            a = _step_length(slope, L, div, gamma)
            trial = None
            if a < 1:
                hcoef, hdiv, ld1, q1, f1 = book.scalars(a, rec)
            else:                                               # the cap: a full evaluation, as the generic solver's
                trial, f1 = capped(rec)
            if not linesearch:
                break
            assert not math.isinf(L), "L is infinite"
            if f1 <= fx + a * slope + a ** gamma * L * div:
                break
            L = L * self.ls_ratio

        self.L = L
        self.Ls[k] = L
        self.done = k + 1
        stop = k > 0 and abs(self.F[k] - self.F[k - 1]) < self.epsilon
        if trial is not None:
            return None, trial, stop
        book.stepped(ld1, q1)
        return (rec.i, a, hcoef, hdiv), None, stop

    def result(self, x):
        e = self.done
        return x, self.F[:e].copy(), self.Ls[:e].copy(), self.T[:e].copy()


class _DescentRun:
    """The host side of one instance of D_opt_FW_descent_step (one copy for the single and the lock-step solver): the
    step of iteration k from the record of the probe before it, the stop test from the record after it."""

    def __init__(self, book, maxitrs, epsilon):
        self.book = book
        self.epsilon = epsilon
        self.F = np.zeros(maxitrs)
        self.G = np.zeros(maxitrs)
        self.T = np.zeros(maxitrs)
        self.k = 0
        self.rec = None

    def first(self, rec, now):
        self.rec = rec
        self.F[0] = self.book.value(rec)
        self.T[0] = now

    def step(self, k):
        """(p, alpha, hcoef, hdiv) of the step of iteration k; the book is advanced here."""
        self.k = k
        self.alpha = 2 / (k + 2)
        hcoef, hdiv, ld1, q1, _ = self.book.scalars(self.alpha, self.rec)
        self.book.stepped(ld1, q1)
        return self.rec.i, self.alpha, hcoef, hdiv

    def probed(self, k, rec, now):
        """The record of the probe behind step k; True when the stop test holds."""
        self.rec = rec
        self.F[k] = self.book.value(rec)
        self.T[k] = now
        return abs(self.F[k] - self.F[k - 1]) < self.epsilon or math.sqrt(rec.sum_w2) < self.epsilon

    def result(self, x):
        e = self.k + 1
        return x, self.F[:e].copy(), self.T[:e].copy(), self.G[:e].copy()


def _capped_trial(obj, xd, p, radius, valued):
    """The capped step a == 1 from the device vector xd on the objective ``obj``: x + 1.0 * (s - x) with the vector
    kernels of the generic solver, and its value by a full evaluation when ``valued``.  Returns (trial, f or None)."""
    vertex = vec_vertex(p, radius, _LMO_FILL, xd.numel(), xd.device)
    towards = vec_axpby(1.0, vertex, -1.0, xd)
    trial = vec_axpby(1.0, xd, 1.0, towards)
    return trial, (obj.func_grad(trial, flag=0) if valued else None)


class _FWDivState(_FWState):
    """The Frank-Wolfe state of one handle plus the book of the Bregman-step solvers (``ld``, ``q``, ``since``)."""

    def __init__(self, f, x0, radius, refresh):
        super().__init__(f, x0)
        self.radius = float(radius)
        self.book = _DivBook(self.m, radius, refresh, self.logdet_gram)

    ld = property(lambda self: self.book.ld)
    q = property(lambda self: self.book.q)
    since = property(lambda self: self.book.since)

    def x_dev(self):
        out = torch.empty(self.n, dtype=torch.float64, device=self.obj.device)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_get_state(self.h, _ptr(out), None, None)
        _lib.check(rc, "accbpg_fw_get_state")
        return out

    def x(self):
        return from_dev(self.x_dev(), self.as_numpy)

    def reinit(self, xd):
        """(H, w, log det) afresh from the device vector xd; a singular Gram matrix is DOptimalObj's ValueError."""
        logdet = C.c_double(0.0)
        with torch.cuda.device(self.obj.device):
            self.lib.accbpg_dopt_set_stream(self.h, _stream())
            rc = self.lib.accbpg_fw_init(self.h, _ptr(xd), C.byref(logdet))
        _lib.check(rc, "accbpg_fw_init")
        self.book.reset(logdet.value)

    def refresh_if_due(self):
        if self.book.refresh_due():
            self.reinit(self.x_dev())

    def probe_div(self):
        rec = _lib.FwDivProbe()
        if self._on_device():
            rc = self.lib.accbpg_fw_div_probe_step(self.h, _LMO_FILL, self.radius, C.byref(rec))
        else:
            with torch.cuda.device(self.obj.device):
                rc = self.lib.accbpg_fw_div_probe_step(self.h, _LMO_FILL, self.radius, C.byref(rec))
        if rc:
            _lib.check(rc, "accbpg_fw_div_probe_step")
        return rec

    def scalars(self, a, rec):
        return self.book.scalars(a, rec)

    def apply_step(self, p, a, hcoef, hdiv):
        """The device side of a rank-one step (the book is the caller's)."""
        if self._on_device():
            rc = self.lib.accbpg_fw_div_apply(self.h, p, a, _LMO_FILL, self.radius, hcoef, hdiv)
        else:
            with torch.cuda.device(self.obj.device):
                rc = self.lib.accbpg_fw_div_apply(self.h, p, a, _LMO_FILL, self.radius, hcoef, hdiv)
        if rc:
            _lib.check(rc, "accbpg_fw_div_apply")

    def apply(self, rec, a, hcoef, hdiv, ld1, q1):
        self.apply_step(rec.i, a, hcoef, hdiv)
        self.book.stepped(ld1, q1)

    def capped(self, rec, valued):
        """(trial, f(trial) or None) of the capped step a == 1 from the current x."""
        return _capped_trial(self.obj, self.x_dev(), rec.i, self.radius, valued)

    # ---- what the device-decided solvers need on top ----
    _snap = None
    _div_steps = None

    def snapshot(self):
        """Keep (x, w, H) as they stand, in buffers of this object (accbpg_fw_get_state: synchronises)."""
        if self._snap is None:
            dev = self.obj.device
            self._snap = (torch.empty(self.n, dtype=torch.float64, device=dev),
                          torch.empty(self.n, dtype=torch.float64, device=dev),
                          torch.empty(self.m, self.m, dtype=torch.float64, device=dev))
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_get_state(self.h, *[_ptr(t) for t in self._snap])
        _lib.check(rc, "accbpg_fw_get_state")

    def restore(self):
        """Back to the last ``snapshot`` (accbpg_fw_set_state: no probe is pending afterwards)."""
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_set_state(self.h, *[_ptr(t) for t in self._snap])
        _lib.check(rc, "accbpg_fw_set_state")

    def run_div(self, mode, L, gamma, ls_ratio, epsilon, k0, F_prev, nsteps):
        """``nsteps`` iterations predicted on the device behind one synchronisation (accbpg_fw_div_run) from the book as
        it stands: the records of the iterations that ran.  A record whose pivot lies outside [0, n) is returned, not
        raised: the replay reaches it in its turn and calls ``bad_div_pivot``."""
        if self._div_steps is None:
            self._div_steps = (_lib.FwDivStep * _lib.FW_RUN_MAX)()
        prm = _lib.FwDivParams(int(mode), 0, int(k0), float(L), float(gamma), float(ls_ratio), float(epsilon),
                               float(self.book.ld), float(self.book.q), float(F_prev))
        nrun = C.c_int(0)
        with torch.cuda.device(self.obj.device):
            rc = self.lib.accbpg_fw_div_run(self.h, _LMO_FILL, self.radius, C.byref(prm), int(nsteps), self._div_steps,
                                            C.byref(nrun))
        recs = [_lib.FwDivStep.from_buffer_copy(self._div_steps[j]) for j in range(nrun.value)]     # (copies: a replay keeps the last probe)
        if rc and not (rc == _lib.ERR_ARG and any(not 0 <= r.probe.i < self.n for r in recs)):
            _lib.check(rc, "accbpg_fw_div_run")
        return recs

    def bad_div_pivot(self):
        """The exception of the sequential solver's probe with such a pivot (the library's last error is still the
        message accbpg_fw_div_run left)."""
        _lib.check(_lib.ERR_ARG, "accbpg_fw_div_probe_step")


def D_opt_FW_div_step(f, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2,
                      verbose=True, verbskip=1, radius=1, refresh=REFRESH_DEFAULT):
    """FW_alg_div_step(f, BurgEntropy(), L, x0, maxitrs, gamma, lmo_simplex(radius), ...) on the D-optimal objective
    at O(mn) per iteration: the state of D_opt_FW (H, w) is kept by rank-one updates, the gradient is -w and every
    line-search trial is a few host scalars.  ``f`` is a matrix or a DOptimalObj.  ``refresh``: the state
    is recomputed from x every that many steps (0: never).  Returns (x, F, Ls, T)."""
    return _drain(D_opt_FW_div_step_steps(f, L, x0, maxitrs, gamma, epsilon, linesearch, ls_ratio, verbose, verbskip,
                                          radius, refresh))


def D_opt_FW_div_step_steps(f, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2,
                            verbose=True, verbskip=1, radius=1, refresh=REFRESH_DEFAULT):
    """Generator form: yields k after each outer iteration, returns D_opt_FW_div_step's tuple."""
    _check_options(L, epsilon, ls_ratio)
    if verbose:
        print("\nFW adaptive algorithm")
        print("     k      F(x)         Lk       time")

    t_start = time.time()
    st = _FWDivState(f, x0, radius, refresh)
    run = _DivStepRun(st.book, L, maxitrs, gamma, epsilon, linesearch, ls_ratio)
    for k in range(maxitrs):
        st.refresh_if_due()
        rec = st.probe_div()
        step, trial, stop = run.decide(k, rec, time.time() - t_start, lambda r: st.capped(r, linesearch))
        if trial is None:
            st.apply_step(*step)
        else:
            st.reinit(trial)
        if verbose and k % verbskip == 0:
            print(f"{k:6d}  {run.F[k]:10.3e}  {run.L:10.3e}  {run.T[k]:6.1f}")
        if stop:
            break
        yield k

    return run.result(st.x())


def D_opt_FW_descent_step(f, x0, maxitrs, epsilon=1e-14, verbose=True, verbskip=1, radius=1, refresh=REFRESH_DEFAULT):
    """FW_alg_descent_step(f, BurgEntropy(), x0, maxitrs, lmo_simplex(radius), ...) on the D-optimal objective at
    O(mn) per iteration, on the state of D_opt_FW_div_step.  Returns (x, F, T, G) with G all zeros."""
    return _drain(D_opt_FW_descent_step_steps(f, x0, maxitrs, epsilon, verbose, verbskip, radius, refresh))


def D_opt_FW_descent_step_steps(f, x0, maxitrs, epsilon=1e-14, verbose=True, verbskip=1, radius=1,
                                refresh=REFRESH_DEFAULT):
    """Generator form: yields k after each iteration, returns D_opt_FW_descent_step's tuple."""
    if verbose:
        print("\nFW descent step size algorithm")
        print("     k      F(x)         alpha_k       time")

    t_start = time.time()
    st = _FWDivState(f, x0, radius, refresh)
    run = _DescentRun(st.book, maxitrs, epsilon)
    run.first(st.probe_div(), time.time() - t_start)

    for k in range(1, maxitrs):
        st.apply_step(*run.step(k))
        st.refresh_if_due()
        stop = run.probed(k, st.probe_div(), time.time() - t_start)

        if verbose and (k % verbskip == 0 or k == 1):
            print(f"{k:6d}  {run.F[k]:10.3e}  {run.alpha:10.3e}  {run.T[k]:6.1f}")

        if stop:
            break
        yield k

    return run.result(st.x())


# ---- the Bregman-step solvers with the line search predicted on the device ----------------------------
# The generators reach the device through a state object alone -- book, refresh_if_due, probe_div, apply_step, capped,
# reinit, snapshot, restore, run_div, bad_div_pivot, x -- (tests/test_fw_div_device_cpu.py drives them with a NumPy
# stand-in) and take every decision in the _DivStepRun / _DescentRun of the sequential solvers: the device predicts a
# chunk (accbpg_fw_div_run), the host replays its records and owns the result.
class _Capped(Exception):
    """The replay of a record met the capped step: that iteration belongs to the sequential path."""


def _replay_capped(rec):
    raise _Capped()


def _same_bits(mine, theirs, fmt):
    return all(struct.pack(f, a) == struct.pack(f, b) or (a != a and b != b) for f, a, b in zip(fmt, mine, theirs))


def _div_chunk(k, maxitrs, sync_every, book, lead=0):
    """Iterations of the chunk that starts at k: ``sync_every`` (None: SYNC_EVERY_DEFAULT), cut at maxitrs, at what one
    call holds and so that no refresh falls inside it (``lead``: steps the chunk applies before its first probe)."""
    S = SYNC_EVERY_DEFAULT if sync_every is None else int(sync_every)
    if S < 1:
        raise ValueError("sync_every must be at least 1")
    S = min(S, maxitrs - k, _lib.FW_RUN_MAX)
    if book.refresh:
        S = min(S, book.refresh - book.since - lead)
    return S


def _device_stats(stats):
    stats = {} if stats is None else stats
    for name in ("chunks", "rollbacks", "handed_back"):
        stats.setdefault(name, 0)
    return stats


def D_opt_FW_div_step_device(f, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, verbose=True,
                             verbskip=1, radius=1, refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT, stats=None):
    """D_opt_FW_div_step with ``sync_every`` iterations per host round trip.  The device predicts the line search of
    every iteration of a chunk with its own log and pow (accbpg_fw_div_run); the host replays the chunk's records
    through ``_DivStepRun.decide`` -- its ld, q, F and Ls are the ones returned -- and compares its (p, a, hcoef, hdiv),
    L and stop decision with the device's bit for bit.  Where they differ (a decision within a rounding of a tie: not an
    error) the state of the chunk's start is restored and the iterations up to that one are redone step by step with
    the host's decisions (``stats["rollbacks"]``); an iteration the device hands back -- the capped step, a failed
    check -- runs on the sequential path (``stats["handed_back"]``); where only the HOST's replay of a record meets the
    cap, the chunk is rolled back and that iteration runs on the sequential path, counted under ``rollbacks`` alone.  A
    chunk never spans a refresh.  Returns
    D_opt_FW_div_step's tuple; x, F, Ls and the iteration count are bit-identical to D_opt_FW_div_step's for every
    argument set; T[k] is the arrival time of the chunk, table rows are printed per chunk.

    gamma == 2 (every driver of the reference): ``** 1.0`` is exact, only log and a ** 2 stand between the device and
    the host, and rollbacks are near-ties.  Other gamma: the step length itself goes through pow, rollbacks may be
    frequent and the form may not pay; the result is the sequential solver's all the same."""
    return _drain(D_opt_FW_div_step_device_steps(f, L, x0, maxitrs, gamma, epsilon, linesearch, ls_ratio, verbose,
                                                 verbskip, radius, refresh, sync_every, stats))


def D_opt_FW_div_step_device_steps(f, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, verbose=True,
                                   verbskip=1, radius=1, refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT,
                                   stats=None):
    """Generator form: yields the last k of each chunk, returns D_opt_FW_div_step_device's tuple."""
    _check_options(L, epsilon, ls_ratio)
    if verbose:
        print("\nFW adaptive algorithm")
        print("     k      F(x)         Lk       time")
    t_start = time.time()
    st = _FWDivState(f, x0, radius, refresh)
    run = _DivStepRun(st.book, L, maxitrs, gamma, epsilon, linesearch, ls_ratio)
    return _div_device_steps(st, run, maxitrs, verbose, verbskip, sync_every, _device_stats(stats), t_start)


def _div_device_steps(st, run, maxitrs, verbose, verbskip, sync_every, stats, t_start):
    """D_opt_FW_div_step_device_steps on a state object and the sequential solver's ``_DivStepRun``."""
    mode = _lib.FW_DIV_LINESEARCH if run.linesearch else _lib.FW_DIV_FIXED_L

    def row(k):
        if verbose and k % verbskip == 0:
            print(f"{k:6d}  {run.F[k]:10.3e}  {run.Ls[k]:10.3e}  {run.T[k]:6.1f}")

    k = 0
    stop = False
    while k < maxitrs and not stop:
        st.refresh_if_due()
        nsteps = _div_chunk(k, maxitrs, sync_every, st.book)
        st.snapshot()
        recs = st.run_div(mode, run.L, run.gamma, run.ls_ratio, run.epsilon, k, run.F[k - 1] if k else 0.0, nsteps)
        now = time.time() - t_start
        stats["chunks"] += 1
        k, stop = _div_replay_records(st, run, recs, k, now, stats, t_start, row, [])
        if not stop:
            yield k - 1

    return run.result(st.x())


def _div_sequential(st, run, k, t_start):
    """One iteration of D_opt_FW_div_step on the state object; True when the stop test holds."""
    st.refresh_if_due()
    rec = st.probe_div()
    step, trial, stop = run.decide(k, rec, time.time() - t_start, lambda r: st.capped(r, run.linesearch))
    if trial is None:
        st.apply_step(*step)
    else:
        st.reinit(trial)
    return stop


def _div_replay_records(st, run, recs, k, now, stats, t_start, row, mine):
    """The host's replay of the records ``recs`` of a chunk from iteration k on, up to and including the first that is
    not an agreed step: that one is redone from the snapshot (a disagreement) or run on the sequential path (a
    hand-back).  ``mine``: the host's steps of the chunk before ``recs``.  Returns (the next k, stop)."""
    stop = False
    for r in recs:
        if r.status == _lib.FW_DIV_HANDED_BACK:                 # nothing applied: the state is that of iteration k
            stats["handed_back"] += 1
            if r.reason == _lib.FW_DIV_HB_PIVOT:
                st.bad_div_pivot()
            stop = _div_sequential(st, run, k, t_start)
        else:
            try:
                step, _, stop = run.decide(k, r.probe, now, _replay_capped)
            except _Capped:
                step = None
            if step is not None and stop == (r.status == _lib.FW_DIV_STOPPED) and _same_bits(
                    step + (run.Ls[k],), (r.probe.i, r.a, r.hcoef, r.hdiv, r.L), "qdddd"):
                mine.append(step)
                row(k)
                k += 1
                if stop:
                    break
                continue
            stats["rollbacks"] += 1                             # redo the chunk up to k with the host's decisions
            st.restore()
            for s in mine:
                st.probe_div()
                st.apply_step(*s)
            if step is None:
                stop = _div_sequential(st, run, k, t_start)
            else:
                st.probe_div()
                st.apply_step(*step)
        row(k)
        k += 1
        break
    return k, stop


def D_opt_FW_descent_step_device(f, x0, maxitrs, epsilon=1e-14, verbose=True, verbskip=1, radius=1,
                                 refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT, stats=None):
    """D_opt_FW_descent_step with ``sync_every`` iterations per host round trip, by the contract of
    ``D_opt_FW_div_step_device``: the device applies the classical steps 2 / (k + 2) of a chunk and predicts the stop
    test, the host replays the records through ``_DescentRun``.  Returns D_opt_FW_descent_step's tuple; x, F, G and the
    iteration count are bit-identical to D_opt_FW_descent_step's."""
    return _drain(D_opt_FW_descent_step_device_steps(f, x0, maxitrs, epsilon, verbose, verbskip, radius, refresh,
                                                     sync_every, stats))


def D_opt_FW_descent_step_device_steps(f, x0, maxitrs, epsilon=1e-14, verbose=True, verbskip=1, radius=1,
                                       refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT, stats=None):
    """Generator form: yields the last k of each chunk, returns D_opt_FW_descent_step_device's tuple."""
    if verbose:
        print("\nFW descent step size algorithm")
        print("     k      F(x)         alpha_k       time")
    t_start = time.time()
    st = _FWDivState(f, x0, radius, refresh)
    run = _DescentRun(st.book, maxitrs, epsilon)
    return _descent_device_steps(st, run, maxitrs, verbose, verbskip, sync_every, _device_stats(stats), t_start)


def _descent_device_steps(st, run, maxitrs, verbose, verbskip, sync_every, stats, t_start):
    """D_opt_FW_descent_step_device_steps on a state object and the sequential solver's ``_DescentRun``."""
    def row(k):
        if verbose and (k % verbskip == 0 or k == 1):
            print(f"{k:6d}  {run.F[k]:10.3e}  {run.alpha:10.3e}  {run.T[k]:6.1f}")

    run.first(st.probe_div(), time.time() - t_start)
    k = 1
    stop = False
    while k < maxitrs and not stop:
        nsteps = _div_chunk(k, maxitrs, sync_every, st.book, lead=1)
        if nsteps < 1:                                          # the refresh falls between this step and its probe
            stop = _descent_sequential(st, run, k, t_start)
            row(k)
            k += 1
            if not stop:
                yield k - 1
            continue
        st.snapshot()
        recs = st.run_div(_lib.FW_DIV_CLASSICAL, 0.0, 0.0, 0.0, run.epsilon, k, run.F[k - 1], nsteps)
        now = time.time() - t_start
        stats["chunks"] += 1
        k, stop = _descent_replay_records(st, run, recs, k, now, stats, t_start, row, [])
        if not stop:
            yield k - 1

    return run.result(st.x())


def _descent_sequential(st, run, k, t_start):
    """One iteration of D_opt_FW_descent_step on the state object; True when the stop test holds."""
    st.apply_step(*run.step(k))
    st.refresh_if_due()
    return run.probed(k, st.probe_div(), time.time() - t_start)


def _descent_replay_records(st, run, recs, k, now, stats, t_start, row, mine):
    """``_div_replay_records`` for the classical step: the record of iteration k holds the step the device applied and
    the probe behind it."""
    stop = False
    for r in recs:
        if r.status == _lib.FW_DIV_HANDED_BACK:                 # nothing applied: the probe before step k is pending
            stats["handed_back"] += 1
            stop = _descent_sequential(st, run, k, t_start)
        else:
            step = run.step(k)
            mine.append(step)
            agree = _same_bits(step[1:], (r.a, r.hcoef, r.hdiv), "ddd")
            if agree:                                           # (else the record's probe saw another state)
                if not 0 <= r.probe.i < st.n:
                    st.bad_div_pivot()
                stop = run.probed(k, r.probe, now)
                agree = stop == (r.status == _lib.FW_DIV_STOPPED)
            if agree:
                row(k)
                k += 1
                if stop:
                    break
                continue
            stats["rollbacks"] += 1                             # redo the chunk up to k with the host's decisions
            st.restore()
            rec = st.probe_div()
            for s in mine:
                st.apply_step(*s)
                rec = st.probe_div()
            stop = run.probed(k, rec, time.time() - t_start)
        row(k)
        k += 1
        break
    return k, stop


# ---- the Bregman-step solvers on the instances of a batch in lock-step --------------------------------
# The generators reach the device through the batch alone -- fw_rows, fw_init, fw_x, fw_div_probe, fw_div_apply and
# fw_div_capped -- and take every decision in the per-instance _DivStepRun / _DescentRun of the sequential solvers.
def _named(i, call, *args):
    """call(*args) for instance i of a batch: what the sequential solver raises, with the instance index in front."""
    try:
        return call(*args)
    except (ValueError, AssertionError) as err:
        raise type(err)("instance %d: %s" % (i, err)) from None


def _div_reinit(batch, X, books, which):
    """Re-initialise the instances ``which`` (a K-mask) from their rows of X, the others staying as they are."""
    logdet = batch.fw_init(X, active=which, named=True)
    for i, on in enumerate(which):
        if on:
            books[i].reset(logdet[i])


def _div_refresh(batch, X, books, active):
    """Those of the active instances whose refresh is due, re-initialised from their own x in one masked call."""
    due = [bool(active[i]) and books[i].refresh_due() for i in range(batch.K)]
    if any(due):
        for i in range(batch.K):
            if due[i]:
                X[i] = batch.fw_x(i, False)
        _div_reinit(batch, X, books, due)


def D_opt_FW_div_step_batch(batch, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1,
                            refresh=REFRESH_DEFAULT):
    """D_opt_FW_div_step on the K instances of a ``DOptimalBatch`` in lock-step: one launch per step kernel covers the
    instances still running and one synchronisation returns all their probe records; a line-search trial is host scalars,
    so instances whose searches take different numbers of trials still share every launch.  ``x0``: one vector or a
    K x n array; ``L``: a scalar or one per instance.  An instance that meets its stop test drops out of the later
    launches; refreshes are per instance; a trial at the cap a == 1 is built and valued on that instance's own handle,
    and an accepted one re-initialises that instance alone.  Silent.  Returns a list of K tuples (x, F, Ls, T), x, F
    and Ls bit-identical to ``D_opt_FW_div_step(batch.instance(i), L_i, x0_i, maxitrs, gamma, ..., verbose=False)``;
    what that raises is raised with "instance i: " in front."""
    return _drain(D_opt_FW_div_step_batch_steps(batch, L, x0, maxitrs, gamma, epsilon, linesearch, ls_ratio, radius,
                                                refresh))


def D_opt_FW_div_step_batch_steps(batch, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1,
                                  refresh=REFRESH_DEFAULT):
    """Generator form of D_opt_FW_div_step_batch: yields k after each lock-step iteration, returns its list."""
    K = batch.K
    Lv = _batch_eps(batch, L)
    for i in range(K):
        _named(i, _check_options, Lv[i], epsilon, ls_ratio)
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    logdet = batch.fw_init(X)
    books = [_DivBook(batch.m, radius, refresh, logdet[i]) for i in range(K)]
    runs = [_DivStepRun(books[i], Lv[i], maxitrs, gamma, epsilon, linesearch, ls_ratio) for i in range(K)]
    active = [True] * K
    steps = [None] * K
    for k in range(maxitrs):
        _div_refresh(batch, X, books, active)
        recs = batch.fw_div_probe(active, radius)
        now = time.time() - t_start
        stepping = [False] * K
        for i in range(K):
            if not active[i]:
                continue
            steps[i], trial, stop = _named(i, runs[i].decide, k, recs[i], now,
                                           lambda r, i=i: batch.fw_div_capped(i, r.i, radius, linesearch))
            if trial is None:
                stepping[i] = True
            else:                                               # the capped step: this instance alone, from the trial
                X[i] = trial
                _div_reinit(batch, X, books, [j == i for j in range(K)])
            active[i] = not stop                                # (the step of the stopping iteration is still taken)
        if any(stepping):
            batch.fw_div_apply(stepping, steps)
        if not any(active):
            break
        yield k
    return [runs[i].result(batch.fw_x(i, as_numpy)) for i in range(K)]


def D_opt_FW_descent_step_batch(batch, x0, maxitrs, epsilon=1e-14, radius=1, refresh=REFRESH_DEFAULT):
    """D_opt_FW_descent_step on the K instances of a ``DOptimalBatch`` in lock-step (see ``D_opt_FW_div_step_batch``).
    Silent.  Returns a list of K tuples (x, F, T, G), x and F bit-identical to
    ``D_opt_FW_descent_step(batch.instance(i), x0_i, maxitrs, ..., verbose=False)``."""
    return _drain(D_opt_FW_descent_step_batch_steps(batch, x0, maxitrs, epsilon, radius, refresh))


def D_opt_FW_descent_step_batch_steps(batch, x0, maxitrs, epsilon=1e-14, radius=1, refresh=REFRESH_DEFAULT):
    """Generator form of D_opt_FW_descent_step_batch: yields k after each lock-step iteration, returns its list."""
    K = batch.K
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    logdet = batch.fw_init(X)
    books = [_DivBook(batch.m, radius, refresh, logdet[i]) for i in range(K)]
    runs = [_DescentRun(books[i], maxitrs, epsilon) for i in range(K)]
    active = [True] * K
    steps = [None] * K
    recs = batch.fw_div_probe(active, radius)
    now = time.time() - t_start
    for i in range(K):
        runs[i].first(recs[i], now)
    for k in range(1, maxitrs):
        for i in range(K):
            if active[i]:
                steps[i] = runs[i].step(k)
        batch.fw_div_apply(active, steps)
        _div_refresh(batch, X, books, active)
        recs = batch.fw_div_probe(active, radius)
        now = time.time() - t_start
        for i in range(K):
            if active[i] and runs[i].probed(k, recs[i], now):
                active[i] = False
        if not any(active):
            break
        yield k
    return [runs[i].result(batch.fw_x(i, as_numpy)) for i in range(K)]


# ---- the lock-step Bregman-step batches with the line search predicted on the device ------------------
# The generators reach the device through the batch alone -- the methods of the 6g solvers plus fw_div_run, fw_snapshot,
# fw_restore, fw_div_replay and bad_div_pivot -- and every instance's records go through the per-record code of the
# single-handle device solvers above (``_div_replay_records`` / ``_descent_replay_records``) on a view of that instance.
REPLAYS = ("c", "python")


class _BatchInstance:
    """Instance i of a batch as the state object the per-record code of the device solvers works on: every call is a
    masked call of the batch on this instance alone, so a roll-back or a hand-back moves no other instance."""

    def __init__(self, batch, i, X, books, radius):
        self.batch, self.i, self.X, self.books, self.radius = batch, i, X, books, radius
        self.book = books[i]
        self.n = batch.n
        self.only = [j == i for j in range(batch.K)]

    def refresh_if_due(self):
        _div_refresh(self.batch, self.X, self.books, self.only)

    def probe_div(self):
        return copy.copy(self.batch.fw_div_probe(self.only, self.radius)[self.i])

    def apply_step(self, p, a, hcoef, hdiv):
        steps = [None] * self.batch.K
        steps[self.i] = (p, a, hcoef, hdiv)
        self.batch.fw_div_apply(self.only, steps)

    def capped(self, rec, valued):
        return self.batch.fw_div_capped(self.i, rec.i, self.radius, valued)

    def reinit(self, trial):
        self.X[self.i] = trial
        _div_reinit(self.batch, self.X, self.books, self.only)

    def restore(self):
        self.batch.fw_restore(self.i)

    def bad_div_pivot(self):
        self.batch.bad_div_pivot(self.i)


def _named_once(i, call, *args):
    """``_named`` for calls that may already have named the instance (the masked re-initialisation does)."""
    try:
        return call(*args)
    except (ValueError, AssertionError) as err:
        head = "instance %d: " % i
        raise type(err)(str(err) if str(err).startswith(head) else head + str(err)) from None


def _no_row(k):
    pass


def _replay_fast_forward(st, prm, recs, pending=None):
    """The C replay of one instance's records (``accbpg_fw_div_replay``) from the book ``prm``; the book is advanced
    past the agreed records.  Returns (agreed, verdict, F, Ls or step lengths, the book as the C side returns it)."""
    agreed, verdict, F, LA, bk = st.batch.fw_div_replay(st.i, prm, recs, pending)
    st.book.ld, st.book.q = bk.ld, bk.q
    st.book.since += agreed
    return agreed, verdict, F, LA, bk


def _div_replay_chunk(st, run, mode, recs, k, now, stats, replay, t_start):
    """One instance's records of a chunk that started at its iteration k: (the next k, stop)."""
    mine = []
    if replay == "c":
        prm = _lib.FwDivParams(mode, 0, k, run.L, run.gamma, run.ls_ratio, run.epsilon, st.book.ld, st.book.q,
                               run.F[k - 1] if k else 0.0)
        agreed, verdict, F, Ls, bk = _replay_fast_forward(st, prm, recs)
        if agreed:
            run.F[k:k + agreed], run.Ls[k:k + agreed], run.T[k:k + agreed] = F, Ls, now
            run.L, run.done = bk.L, k + agreed
            k += agreed
        if verdict in (_lib.FW_DIV_RP_END, _lib.FW_DIV_RP_STOP):
            return k, verdict == _lib.FW_DIV_RP_STOP
        if verdict in (_lib.FW_DIV_RP_HOST_HB, _lib.FW_DIV_RP_DISAGREE):     # a roll-back redoes the agreed steps
            for j in range(agreed):
                r = recs[j]
                mine.append((r.probe.i, r.a, r.hcoef, r.hdiv))
        recs = [recs[agreed]]
    return _div_replay_records(st, run, recs, k, now, stats, t_start, _no_row, mine)


def _descent_replay_chunk(st, run, recs, k, now, stats, replay, t_start):
    """``_div_replay_chunk`` for the classical step; the probe before the chunk's first step is ``run.rec``."""
    mine = []
    if replay == "c":
        prm = _lib.FwDivParams(_lib.FW_DIV_CLASSICAL, 0, k, 0.0, 0.0, 0.0, run.epsilon, st.book.ld, st.book.q, run.F[k - 1])
        agreed, verdict, F, alphas, bk = _replay_fast_forward(st, prm, recs, run.rec)
        if agreed:
            if verdict in (_lib.FW_DIV_RP_HOST_HB, _lib.FW_DIV_RP_DISAGREE, _lib.FW_DIV_RP_PIVOT):
                prev = run.rec                                  # a roll-back redoes the agreed steps
                for j in range(agreed):
                    r = recs[j]
                    mine.append((prev.i, r.a, r.hcoef, r.hdiv))
                    prev = r.probe
            run.F[k:k + agreed], run.T[k:k + agreed] = F, now
            run.k, run.alpha, run.rec = k + agreed - 1, float(alphas[-1]), recs[agreed - 1].probe
            k += agreed
        if verdict in (_lib.FW_DIV_RP_END, _lib.FW_DIV_RP_STOP):
            return k, verdict == _lib.FW_DIV_RP_STOP
        recs = [recs[agreed]]
    return _descent_replay_records(st, run, recs, k, now, stats, t_start, _no_row, mine)


def _batch_device_setup(batch, x0, radius, refresh, replay):
    if replay not in REPLAYS:
        raise ValueError("replay must be one of %s" % (REPLAYS,))
    X, as_numpy = batch.fw_rows(x0)
    logdet = batch.fw_init(X)
    books = [_DivBook(batch.m, radius, refresh, logdet[i]) for i in range(batch.K)]
    return X, as_numpy, books, [_BatchInstance(batch, i, X, books, radius) for i in range(batch.K)]


def D_opt_FW_div_step_batch_device(batch, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2, radius=1,
                                   refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT, stats=None, replay="c"):
    """D_opt_FW_div_step_batch with ``sync_every`` iterations per host round trip, by the contract of
    ``D_opt_FW_div_step_device`` per instance: the device predicts a chunk of every running instance in lock-step
    (accbpg_dopt_batch_fw_div_run), the host replays each instance's records -- ``replay="c"``: the agreed records in C
    (accbpg_fw_div_replay), the first that is not an agreed step through the Python text; ``replay="python"``: every
    record through the Python text -- and owns the result.  A chunk is as long as the shortest of the running
    instances' own limits (maxitrs, its refresh); a disagreement restores and redoes that instance alone, a hand-back
    runs that iteration of that instance on the sequential path, and the instances then carry different iteration
    numbers.  ``stats``: ``chunks`` (per instance and call), ``rollbacks``, ``handed_back``, summed over the instances.
    Silent.  Returns a list of K tuples (x, F, Ls, T); x, F, Ls and the iteration count of instance i are bit-identical
    to ``D_opt_FW_div_step(batch.instance(i), L_i, x0_i, maxitrs, gamma, ...)``, and what that raises is raised with
    "instance i: " in front."""
    return _drain(D_opt_FW_div_step_batch_device_steps(batch, L, x0, maxitrs, gamma, epsilon, linesearch, ls_ratio,
                                                       radius, refresh, sync_every, stats, replay))


def D_opt_FW_div_step_batch_device_steps(batch, L, x0, maxitrs, gamma, epsilon=1e-14, linesearch=True, ls_ratio=2,
                                         radius=1, refresh=REFRESH_DEFAULT, sync_every=SYNC_EVERY_DEFAULT, stats=None,
                                         replay="c"):
    """Generator form: yields the largest iteration number reached after each chunk, returns the list."""
    K = batch.K
    Lv = _batch_eps(batch, L)
    for i in range(K):
        _named(i, _check_options, Lv[i], epsilon, ls_ratio)
    stats = _device_stats(stats)
    t_start = time.time()
    X, as_numpy, books, insts = _batch_device_setup(batch, x0, radius, refresh, replay)
    runs = [_DivStepRun(books[i], Lv[i], maxitrs, gamma, epsilon, linesearch, ls_ratio) for i in range(K)]
    mode = _lib.FW_DIV_LINESEARCH if linesearch else _lib.FW_DIV_FIXED_L
    ks = [0] * K
    running = [maxitrs > 0] * K
    while any(running):
        _div_refresh(batch, X, books, running)
        nsteps = min(_div_chunk(ks[i], maxitrs, sync_every, books[i]) for i in range(K) if running[i])
        batch.fw_snapshot(running)
        params = [(ks[i], runs[i].L, gamma, ls_ratio, epsilon, books[i].ld, books[i].q,
                   runs[i].F[ks[i] - 1] if ks[i] else 0.0) if running[i] else None for i in range(K)]
        recs = batch.fw_div_run(mode, params, nsteps, running, radius)
        now = time.time() - t_start
        for i in range(K):
            if running[i]:
                stats["chunks"] += 1
                ks[i], stop = _named_once(i, _div_replay_chunk, insts[i], runs[i], mode, recs[i], ks[i], now, stats,
                                          replay, t_start)
                running[i] = not stop and ks[i] < maxitrs
        yield max(ks) - 1
    return [runs[i].result(batch.fw_x(i, as_numpy)) for i in range(K)]


def D_opt_FW_descent_step_batch_device(batch, x0, maxitrs, epsilon=1e-14, radius=1, refresh=REFRESH_DEFAULT,
                                       sync_every=SYNC_EVERY_DEFAULT, stats=None, replay="c"):
    """D_opt_FW_descent_step_batch with ``sync_every`` iterations per host round trip (see
    ``D_opt_FW_div_step_batch_device``).  Silent.  Returns a list of K tuples (x, F, T, G); x, F, G and the iteration
    count of instance i are bit-identical to ``D_opt_FW_descent_step(batch.instance(i), x0_i, maxitrs, ...)``."""
    return _drain(D_opt_FW_descent_step_batch_device_steps(batch, x0, maxitrs, epsilon, radius, refresh, sync_every,
                                                           stats, replay))


def D_opt_FW_descent_step_batch_device_steps(batch, x0, maxitrs, epsilon=1e-14, radius=1, refresh=REFRESH_DEFAULT,
                                             sync_every=SYNC_EVERY_DEFAULT, stats=None, replay="c"):
    """Generator form: yields the largest iteration number reached after each chunk, returns the list."""
    K = batch.K
    stats = _device_stats(stats)
    t_start = time.time()
    X, as_numpy, books, insts = _batch_device_setup(batch, x0, radius, refresh, replay)
    runs = [_DescentRun(books[i], maxitrs, epsilon) for i in range(K)]
    first = batch.fw_div_probe([True] * K, radius)
    now = time.time() - t_start
    for i in range(K):
        runs[i].first(copy.copy(first[i]), now)
    ks = [1] * K
    running = [maxitrs > 1] * K
    while any(running):
        limit = [_div_chunk(ks[i], maxitrs, sync_every, books[i], lead=1) if running[i] else 0 for i in range(K)]
        due = [running[i] and limit[i] < 1 for i in range(K)]   # the refresh falls between this step and its probe
        if any(due):
            for i in range(K):
                if due[i]:
                    stop = _named_once(i, _descent_sequential, insts[i], runs[i], ks[i], t_start)
                    ks[i] += 1
                    running[i] = not stop and ks[i] < maxitrs
            yield max(ks) - 1
            continue
        nsteps = min(limit[i] for i in range(K) if running[i])
        batch.fw_snapshot(running)
        params = [(ks[i], 0.0, 0.0, 0.0, epsilon, books[i].ld, books[i].q, runs[i].F[ks[i] - 1]) if running[i] else None
                  for i in range(K)]
        recs = batch.fw_div_run(_lib.FW_DIV_CLASSICAL, params, nsteps, running, radius)
        now = time.time() - t_start
        for i in range(K):
            if running[i]:
                stats["chunks"] += 1
                ks[i], stop = _named_once(i, _descent_replay_chunk, insts[i], runs[i], recs[i], ks[i], now, stats, replay,
                                          t_start)
                running[i] = not stop and ks[i] < maxitrs
        yield max(ks) - 1
    return [runs[i].result(batch.fw_x(i, as_numpy)) for i in range(K)]
