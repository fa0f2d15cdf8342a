"""Batches of independent instances on one GPU (BASELINE config 4: many D_opt_design(512,8192)
instances per device).

Small instances are latency-bound (a 512 x 512 Cholesky is a chain of 512 pivots on a handful of
CUs), so one instance cannot fill the chip.  Instances are independent and take different
line-search / stopping paths, so instead of a masked lock-step batch each instance runs the
ordinary solver loop from its own host thread on its own HIP stream; kernels of different
instances overlap on the device.  ctypes releases the GIL while a call waits on its stream.
Every instance owns its D-optimal handle; the length-n kernels keep their scratch per thread.
"""
from __future__ import annotations

import ctypes as C
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from .algorithms import _drain
from .functions import DOptimalObj, _ptr, _stream, from_dev, to_dev
from .solver_runs import NEEDS_VALUE, RETRY, _ABDARun, _ABPGRun, _BPGRun, _ExpoRun, _GainRun


class _FwDivRecords:
    """The records of one instance of a ``fw_div_run`` call: ``count`` entries of a ctypes array of ``_lib.FwDivStep``
    from ``first`` on.  The buffer belongs to the batch and the next call overwrites it: indexing copies a record out."""

    def __init__(self, array, first, count):
        self.array, self.first, self.count = array, first, count

    def __len__(self):
        return self.count

    def __getitem__(self, j):
        if not 0 <= j < self.count:
            raise IndexError(j)
        return _lib.FwDivStep.from_buffer_copy(self.array[self.first + j])

    def pivot(self, j):
        return self.array[self.first + j].probe.i

    def address(self):
        return C.addressof(self.array) + self.first * C.sizeof(_lib.FwDivStep)


def _lib_fw_div_replay(lib, prm, n, m, fill, radius, recs, pending=None):
    """``accbpg_fw_div_replay`` on the records ``recs`` (a ``_FwDivRecords``, or any sequence of objects with the fields
    of ``_lib.FwDivStep``) from the book ``prm``; see ``DOptimalBatch.fw_div_replay``."""
    nrun = len(recs)
    classical = prm.mode == _lib.FW_DIV_CLASSICAL
    if isinstance(recs, _FwDivRecords) and not classical:
        steps = C.cast(recs.address(), C.POINTER(_lib.FwDivStep))
    else:                                           # (classical: the pending probe in front of the records)
        lead = 1 if classical else 0
        arr = (_lib.FwDivStep * (nrun + lead))()
        if classical:
            for name, _ in _lib.FwDivProbe._fields_:
                setattr(arr[0].probe, name, getattr(pending, name))
        if isinstance(recs, _FwDivRecords):
            C.memmove(C.addressof(arr) + lead * C.sizeof(_lib.FwDivStep), recs.address(), nrun * C.sizeof(_lib.FwDivStep))
        else:
            for j, r in enumerate(recs):
                s = arr[lead + j]
                for name, _ in _lib.FwDivProbe._fields_:
                    setattr(s.probe, name, getattr(r.probe, name))
                for name in ("L", "a", "hcoef", "hdiv", "ld1", "q1", "f1", "trials", "status", "reason"):
                    setattr(s, name, getattr(r, name))
        steps = arr
    F = np.empty(nrun)
    LA = np.empty(nrun)
    book = _lib.FwDivParams()
    agreed, verdict = C.c_int(0), C.c_int(0)
    rc = lib.accbpg_fw_div_replay(C.byref(prm), n, m, fill, radius, steps, nrun,
                                  F.ctypes.data_as(C.POINTER(C.c_double)), LA.ctypes.data_as(C.POINTER(C.c_double)),
                                  C.byref(book), C.byref(agreed), C.byref(verdict))
    _lib.check(rc, "accbpg_fw_div_replay")
    return agreed.value, verdict.value, F[:agreed.value], LA[:agreed.value], book


class DOptimalBatch:
    """K D-optimal objectives of ONE shape evaluated together (C-ABI ``accbpg_dopt_batch_*``): every call covers the
    active instances with one launch per kernel family and one readback.  Vectors are K x n CUDA tensors, row i =
    instance i.  The arithmetic of instance i is bit for bit that of ``self.instance(i)`` (a ``DOptimalObj`` on the
    same handle), so a lock-step batch and a loop over the instances give identical results."""

    def __init__(self, matrices):
        self._Vs = [to_dev(V)[0] for V in matrices]
        assert self._Vs, "DOptimalBatch: no instances"
        self.K = len(self._Vs)
        self.m, self.n = self._Vs[0].shape
        for V in self._Vs:
            assert V.shape == (self.m, self.n) and V.stride(0) == self._Vs[0].stride(0), \
                "DOptimalBatch: instances must have one shape and one row stride"
        self.device = self._Vs[0].device
        self._lib = _lib.load()
        ptrs = (C.c_void_p * self.K)(*[V.data_ptr() for V in self._Vs])
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_create(ptrs, self.K, self.m, self.n, self._Vs[0].stride(0), _stream(),
                                                    C.byref(h))
        _lib.check(rc, "accbpg_dopt_batch_create")
        self._h = h
        self.fused = bool(self._lib.accbpg_dopt_batch_is_fused(h))
        self.chunk = int(self._lib.accbpg_dopt_batch_chunk(h))      # instances one launch covers
        self.calls = {"value": 0, "grad": 0}        # per instance-evaluation, as DOptimalObj counts them
        self._views = {}
        # host arrays of the lock-step Frank-Wolfe calls (probe records; p, xscale, xadd, hcoef, hdiv of an update)
        self._fw_probes = (_lib.FwProbe * self.K)()
        self._fw_args = ((C.c_int64 * self.K)(),) + tuple((C.c_double * self.K)() for _ in range(4))
        self._fw_steps = None                       # K x FW_RUN_MAX records of fw_run (allocated by the first call)
        self._fw_div_probes = (_lib.FwDivProbe * self.K)()      # records of fw_div_probe
        self._fw_div_radius = 1.0                   # ... and the vertex value of the last one (fw_div_apply steps towards it)
        self._fw_bad_pivot = ""                     # the library's message of the last fw_run that returned a status 2
        self._fw_div_steps = None                   # K x FW_RUN_MAX records of fw_div_run (allocated by the first call)
        self._fw_bad_div_pivot = ""                 # the library's message of the last fw_div_run with such a record
        self._fw_snaps = {}                         # instance -> (x, w, H) of its last fw_snapshot

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.accbpg_dopt_batch_destroy(h)
            except Exception:
                pass
            self._h = None

    def instance(self, i):
        """Instance i as an ordinary objective on the batch's own handle (same plans, same kernels)."""
        if i not in self._views:
            sub = C.c_void_p(self._lib.accbpg_dopt_batch_instance(self._h, int(i)))
            view = DOptimalObj(self._Vs[i], _borrowed=(sub, self))
            view.overlap_values(False)
            self._views[i] = view
        return self._views[i]

    # ---- kernel-time accounting used by bench.py (rides on instance 0's slots of this batch and of its twin) ----
    def _handles0(self):
        hs = [C.c_void_p(self._lib.accbpg_dopt_batch_instance(self._h, 0))]
        twin = getattr(self, "_twin", None)
        if twin is not None:
            hs.append(C.c_void_p(self._lib.accbpg_dopt_batch_instance(twin._h, 0)))
        return hs

    def profile(self, enable=True):
        """HIP-event timing of every batched launch on the stream it is launched on (one event pair per kernel family
        and launch)."""
        self._prof = bool(enable)
        for h in self._handles0():
            self._lib.accbpg_dopt_profile_enable(h, 1 if enable else 0)
            self._lib.accbpg_dopt_profile_reset(h)

    def profile_read(self):
        out = {}
        for idx, name in enumerate(["gram", "cholesky", "trtri", "grad", "gram_fixup", "fw_vpass"]):
            tot, num = 0.0, 0
            for h in self._handles0():
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                self._lib.accbpg_dopt_profile_read(h, idx, C.byref(ms), C.byref(cnt))
                tot, num = tot + ms.value, num + cnt.value
            out[name] = (tot, num)
        return out

    def _mask(self, active):
        if active is None:
            return None, list(range(self.K))
        arr = (C.c_int * self.K)(*[1 if a else 0 for a in active])
        return arr, [i for i in range(self.K) if active[i]]

    def _rows(self, **tensors):
        """The K x n operands (other than func_grad's X, whose row stride is passed) cross the C-ABI with row stride n:
        refuse any that is laid out otherwise instead of letting the kernels misread it."""
        for name, T in tensors.items():
            if T is None:
                continue
            if not (isinstance(T, torch.Tensor) and T.is_cuda and T.dtype == torch.float64
                    and tuple(T.shape) == (self.K, self.n) and T.stride(1) == 1 and (self.K == 1 or T.stride(0) == self.n)):
                raise ValueError("DOptimalBatch: %s must be a K x n float64 device tensor with row stride n (got shape %s, "
                                 "strides %s)" % (name, tuple(getattr(T, "shape", ())),
                                                  T.stride() if isinstance(T, torch.Tensor) else None))

    @staticmethod
    def _raise(status, idx, what, assert_msg):
        for i in idx:
            if status[i] != _lib.OK:
                _lib.check(status[i], "%s (instance %d)" % (what, i), assert_msg)

    def func_grad(self, X, flag=2, active=None, out=None):
        """(f, G): f a length-K NumPy array (entries of inactive instances are nan), G a K x n tensor (rows of
        inactive instances are left unwritten; `out`: an existing tensor for them); flag 0 returns f only, flag 1 G
        only."""
        assert X.shape == (self.K, self.n) and X.is_cuda and X.dtype == torch.float64 and X.stride(1) == 1
        mask, idx = self._mask(active)
        f = (C.c_double * self.K)(*([float("nan")] * self.K))
        st = (C.c_int * self.K)()
        G = None
        if flag != 0:
            self._rows(out=out)
            G = out if out is not None else torch.empty(self.K, self.n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_func_grad(self._h, _ptr(X), X.stride(0), mask, int(flag), f, _ptr(G),
                                                       self.n, st)
        _lib.check(rc, "accbpg_dopt_batch_func_grad")
        self._raise(st, idx, "accbpg_dopt_batch_func_grad", "DOptimalObj: x needs to be nonnegative")
        self.calls["value" if flag == 0 else "grad"] += len(idx)
        fv = np.array(f[:], dtype=np.float64)
        if flag == 0:
            return fv
        return G if flag == 1 else (fv, G)

    # ---- value evaluations beside the gradient evaluations: a second batch over the same matrices, own stream ----
    def value_async(self, X, active=None):
        """Start f(X[i]) for the active instances on a side stream (a twin batch over the same matrices) and
        return a ticket for ``value_wait``.  Same kernels, same plans: the values are those of ``func_grad(X, 0)``."""
        twin = getattr(self, "_twin", None)
        if twin is None:
            twin = self._twin = DOptimalBatch(self._Vs)
            with torch.cuda.device(self.device):
                self._side = torch.cuda.Stream(device=self.device)
        mask, idx = self._mask(active)
        with torch.cuda.device(self.device):
            self._side.wait_stream(torch.cuda.current_stream())          # X is produced on the caller's stream
            self._lib.accbpg_dopt_batch_set_stream(twin._h, C.c_void_p(self._side.cuda_stream))
            rc = self._lib.accbpg_dopt_batch_func_grad_begin(twin._h, _ptr(X), X.stride(0), mask, 0, None, self.n)
        _lib.check(rc, "accbpg_dopt_batch_func_grad_begin")
        return (X, idx)                                                   # the ticket keeps X alive

    def value_wait(self, ticket):
        _, idx = ticket
        f = (C.c_double * self.K)(*([float("nan")] * self.K))
        st = (C.c_int * self.K)()
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_func_grad_end(self._twin._h, f, st)
        _lib.check(rc, "accbpg_dopt_batch_func_grad_end")
        self._raise(st, idx, "accbpg_dopt_batch_func_grad", "DOptimalObj: x needs to be nonnegative")
        self.calls["value"] += len(idx)
        return np.array(f[:], dtype=np.float64)

    def prox(self, Y, G, Ls, eps, active=None, out=None):
        """Row i: BurgEntropySimplex(eps).div_prox_map(Y[i], G[i], Ls[i]) (Y None: prox_map).  Only the rows of the
        active instances are written (`out`: an existing K x n tensor to write them into)."""
        self._rows(Y=Y, G=G, out=out)
        mask, idx = self._mask(active)
        Lc = (C.c_double * self.K)(*[float(v) for v in Ls])
        st = (C.c_int * self.K)()
        if out is None:
            out = torch.empty(self.K, self.n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_burg_simplex_div_prox(self._h, _ptr(Y), _ptr(G), self.n, Lc, float(eps),
                                                                   _ptr(out), mask, st, None)
        _lib.check(rc, "accbpg_dopt_batch_burg_simplex_div_prox")
        self._raise(st, idx, "accbpg_dopt_batch_burg_simplex_div_prox", "Either y or L is not positive.")
        return out

    def avg_prox(self, Gavg, G, wgt, csum, Lc, eps, active=None, out_avg=None, out=None, info=False):
        """ABDA's dual-averaging step (accbpg/algorithms.py:483-485), one launch for the active instances.  Returns
        (Gavg_new, Z): row i of Gavg_new = Gavg[i] + wgt[i] * G[i], row i of Z =
        BurgEntropySimplex(eps).prox_map(Gavg_new[i] / csum[i], Lc[i]) -- bit for bit ``vec_axpby(1.0, Gavg[i], wgt[i],
        G[i])``, ``vec_div_scalar`` and ``prox_map`` in a row.  Lc[i] is L / csum[i] as the caller computed it.  Only the
        rows of the active instances are written (`out_avg`, `out`: existing K x n tensors for them; `out_avg` must not be
        Gavg).  Nothing is read back, unless `info` asks for ``self.last_info[i]`` = (bisection steps, Newton steps) of
        the active instances i."""
        self._rows(Gavg=Gavg, G=G, out_avg=out_avg, out=out)
        if out_avg is not None and (out_avg is Gavg or out_avg.data_ptr() == Gavg.data_ptr()):
            raise ValueError("DOptimalBatch.avg_prox: out_avg must not be Gavg (the sum is read and written in one pass)")
        mask, idx = self._mask(active)
        vals = [(C.c_double * self.K)(*[float(v) for v in seq]) for seq in (wgt, csum, Lc)]
        st = (C.c_int * self.K)()
        steps = (C.c_int * (2 * self.K))() if info else None
        new = lambda: torch.empty(self.K, self.n, dtype=torch.float64, device=self.device)
        out_avg = new() if out_avg is None else out_avg
        out = new() if out is None else out
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_burg_simplex_avg_prox(self._h, _ptr(Gavg), _ptr(G), self.n, vals[0], vals[1],
                                                                   vals[2], float(eps), _ptr(out_avg), _ptr(out), mask, st,
                                                                   steps)
        _lib.check(rc, "accbpg_dopt_batch_burg_simplex_avg_prox")
        self._raise(st, idx, "accbpg_dopt_batch_burg_simplex_avg_prox", "BergEntropySimplex prox_map only takes positive L.")
        if info:
            self.last_info = {i: (steps[2 * i], steps[2 * i + 1]) for i in idx}
        return out_avg, out

    def ls_terms(self, G, X, Y, Z=None, Z1=None, active=None):
        """K x 3 NumPy array: (<g, x-y>, D(x,y), D(z,z1)) per instance."""
        self._rows(G=G, X=X, Y=Y, Z=Z, Z1=Z1)
        mask, idx = self._mask(active)
        out = (C.c_double * (3 * self.K))()
        st = (C.c_int * self.K)()
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_ls_terms(self._h, _ptr(G), _ptr(X), _ptr(Y), _ptr(Z), _ptr(Z1), self.n, mask,
                                                      out, st)
        _lib.check(rc, "accbpg_dopt_batch_ls_terms")
        self._raise(st, idx, "accbpg_dopt_batch_ls_terms", "Entries of x or y not positive.")
        return np.array(out[:], dtype=np.float64).reshape(self.K, 3)

    def axpby(self, a, X, b, Z, active=None, out=None):
        """Row i: a[i]*X[i] + b[i]*Z[i] with NumPy's rounding; only the rows of the active instances are written."""
        self._rows(X=X, Z=Z, out=out)
        mask, _ = self._mask(active)
        av = (C.c_double * self.K)(*[float(v) for v in a])
        bv = (C.c_double * self.K)(*[float(v) for v in b])
        if out is None:
            out = torch.empty(self.K, self.n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_axpby(self._h, av, _ptr(X), bv, _ptr(Z), self.n, mask, _ptr(out))
        _lib.check(rc, "accbpg_dopt_batch_axpby")
        return out

    def kyinit_picks(self, B, Q_out=None):
        """Row i: the 2m indices of instance i's Kumar-Yildirim start for its m directions B[i] (K x m x m;
        accbpg_dopt_batch_kyinit): the K instances in lock-step, all m steps on the device, one synchronisation.
        ``Q_out``: optional K x m x m fp64 device tensor that receives the orthonormal directions, Q_out[i, j] =
        instance i's Q[:, j].  Bit for bit ``self.instance(i).kyinit_picks(B[i], Q_out[i])``."""
        Bd, _ = to_dev(B)
        assert Bd.shape == (self.K, self.m, self.m), "kyinit_picks: B must be K x m x m"
        if Q_out is not None:
            assert Q_out.is_cuda and Q_out.dtype == torch.float64 and Q_out.is_contiguous() \
                and Q_out.shape == (self.K, self.m, self.m), \
                "kyinit_picks: Q_out must be a contiguous K x m x m fp64 device tensor"
        picked = np.empty((self.K, 2 * self.m), dtype=np.int64)
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_kyinit(self._h, _ptr(Bd), picked.ctypes.data_as(C.POINTER(C.c_int64)),
                                                    _ptr(Q_out))
        _lib.check(rc, "accbpg_dopt_batch_kyinit")
        return picked


    # ---- Frank-Wolfe steps in lock-step (C-ABI ``accbpg_dopt_batch_fw_*``); the state lives in the instance handles ----
    def _inst_h(self, i):
        return self.instance(i)._h

    def fw_rows(self, x0):
        """x0 (one vector or K x n, NumPy or torch) as the K x n device tensor ``fw_init`` takes, and whether it came as
        NumPy."""
        from .D_opt_alg import _batch_x0
        return _batch_x0(self, x0)

    def fw_init(self, X0, active=None, named=False):
        """``accbpg_fw_init`` for the active instances from the rows of X0 (K x n); returns log det(V_i diag(x0_i) V_i^T)
        per instance (nan for inactive ones).  A singular instance raises as the single solver does; ``named``: with
        "instance i: " in front."""
        self._rows(X0=X0)
        mask, idx = self._mask(active)
        ld = (C.c_double * self.K)(*([float("nan")] * self.K))
        st = (C.c_int * self.K)()
        with torch.cuda.device(self.device):
            self._lib.accbpg_dopt_batch_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_batch_fw_init(self._h, _ptr(X0), self.n, mask, ld, st)
        _lib.check(rc, "accbpg_dopt_batch_fw_init")
        if named:
            for i in idx:
                try:
                    _lib.check(st[i], "accbpg_dopt_batch_fw_init")
                except (ValueError, AssertionError) as err:
                    raise type(err)("instance %d: %s" % (i, err)) from None
        self._raise(st, idx, "accbpg_dopt_batch_fw_init", None)
        return list(ld)

    def fw_probe(self, away, active=None):
        """One probe of the active instances: one launch chain, one synchronisation.  Returns the K records
        (``_lib.FwProbe``; those of inactive instances are stale), ``logdet_H`` nan."""
        mask, _ = self._mask(active)
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_probe(self._h, int(away), mask, self._fw_probes)
        if rc:
            _lib.check(rc, "accbpg_dopt_batch_fw_probe")
        return self._fw_probes

    def fw_update(self, active, updates):
        """One rank-one update per active instance: updates[i] = (p, xscale, xadd, hcoef, hdiv)."""
        mask, idx = self._mask(active)
        p, xs, xa, hc, hd = self._fw_args
        for i in idx:
            p[i], xs[i], xa[i], hc[i], hd[i] = updates[i]
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_update(self._h, mask, p, xs, xa, hc, hd)
        if rc:
            _lib.check(rc, "accbpg_dopt_batch_fw_update")

    def fw_div_probe(self, active=None, radius=1):
        """One Bregman-step probe of the active instances (``accbpg_dopt_batch_fw_div_probe`` with the simplex LMO's
        vertex of this radius): one launch chain, one synchronisation.  Returns the K records (``_lib.FwDivProbe``; those
        of inactive instances are stale).  The direction of each instance's step stays in its handle for
        ``fw_div_apply``."""
        from .D_opt_alg import _LMO_FILL
        mask, _ = self._mask(active)
        self._fw_div_radius = float(radius)
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_div_probe(self._h, _LMO_FILL, self._fw_div_radius, mask,
                                                          self._fw_div_probes)
        if rc:
            _lib.check(rc, "accbpg_dopt_batch_fw_div_probe")
        return self._fw_div_probes

    def fw_div_apply(self, active, applies):
        """One step x + a (s - x) per active instance towards the vertex of its last ``fw_div_probe``: applies[i] =
        (p, a, hcoef, hdiv) with p that probe's index.  Refused for all if any instance's state moved since its probe.
        Does not synchronise."""
        from .D_opt_alg import _LMO_FILL
        mask, idx = self._mask(active)
        p, a, _, hc, hd = self._fw_args
        for i in idx:
            p[i], a[i], hc[i], hd[i] = applies[i]
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_div_apply(self._h, mask, p, a, _LMO_FILL, self._fw_div_radius, hc, hd)
        if rc:
            _lib.check(rc, "accbpg_dopt_batch_fw_div_apply")

    def fw_div_capped(self, i, p, radius, valued):
        """The capped step a == 1 of instance i towards the vertex at p, on that instance's own handle: (trial, f(trial))
        as the sequential solver forms them; f is None unless ``valued``."""
        from .D_opt_alg import _capped_trial
        return _capped_trial(self.instance(i), self.fw_x(i, False), p, radius, valued)

    # ---- what the device-decided Bregman-step batches need on top ----
    def fw_div_run(self, mode, params, nsteps, active=None, radius=1):
        """``nsteps`` iterations of the active instances predicted on the device behind one synchronisation
        (``accbpg_dopt_batch_fw_div_run``).  params[i] = (k0, L, gamma, ls_ratio, epsilon, ld, q, F_prev) of instance i:
        its own iteration number and the host's exact book.  Returns a list of K entries: for an active instance the
        records of the iterations that ran (a ``_FwDivRecords`` over a buffer the next call overwrites; indexing copies
        a record out), None for an inactive one.  A record whose pivot lies outside [0, n) is returned, not raised: the
        replay reaches it in its turn and calls ``bad_div_pivot``."""
        from .D_opt_alg import _LMO_FILL
        mask, idx = self._mask(active)
        K, nsteps = self.K, int(nsteps)
        if self._fw_div_steps is None:
            self._fw_div_steps = (_lib.FwDivStep * (K * _lib.FW_RUN_MAX))()
            self._fw_div_prm = (_lib.FwDivParams * K)()
        prm = self._fw_div_prm
        for i in idx:
            k0, L, gamma, ls_ratio, epsilon, ld, q, F_prev = params[i]
            prm[i] = _lib.FwDivParams(int(mode), 0, int(k0), float(L), float(gamma), float(ls_ratio), float(epsilon),
                                      float(ld), float(q), float(F_prev))
        nrun = (C.c_int * K)()
        self._fw_div_radius = float(radius)
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_div_run(self._h, _LMO_FILL, self._fw_div_radius, prm, nsteps, mask,
                                                        self._fw_div_steps, nrun)
        out = [None] * K
        for i in idx:
            out[i] = _FwDivRecords(self._fw_div_steps, i * _lib.FW_RUN_MAX, nrun[i])
        if rc:
            bad = [i for i in idx if any(not 0 <= out[i].pivot(j) < self.n for j in range(nrun[i]))]
            if not (rc == _lib.ERR_ARG and bad):
                _lib.check(rc, "accbpg_dopt_batch_fw_div_run")
            self._fw_bad_div_pivot = _lib.last_error()          # (kept for bad_div_pivot)
        return out

    def fw_div_replay(self, i, prm, recs, pending=None):
        """The host's replay of instance i's records in C (``accbpg_fw_div_replay``) from the book ``prm`` (a
        ``_lib.FwDivParams``); ``pending``: in the classical mode, the probe record that was pending when the chunk
        started.  Returns (agreed, verdict, F, L_or_alpha, book) with F and L_or_alpha NumPy arrays of ``agreed``
        entries and book the ``_lib.FwDivParams`` BEFORE record ``agreed``."""
        from .D_opt_alg import _LMO_FILL
        return _lib_fw_div_replay(self._lib, prm, self.n, self.m, _LMO_FILL, self._fw_div_radius, recs, pending)

    def bad_div_pivot(self, i):
        """The exception of the sequential solver's probe of instance i with a pivot outside [0, n), with the message of
        the ``fw_div_run`` call that returned the record."""
        raise ValueError("instance %d: accbpg_fw_div_probe_step: bad argument (%s)" % (i, self._fw_bad_div_pivot))

    def fw_snapshot(self, active=None):
        """Keep (x, w, H) of the active instances as they stand, in buffers of the batch (``accbpg_fw_get_state`` on the
        instance handles: synchronises)."""
        _, idx = self._mask(active)
        with torch.cuda.device(self.device):
            for i in idx:
                if i not in self._fw_snaps:
                    self._fw_snaps[i] = (torch.empty(self.n, dtype=torch.float64, device=self.device),
                                         torch.empty(self.n, dtype=torch.float64, device=self.device),
                                         torch.empty(self.m, self.m, dtype=torch.float64, device=self.device))
                rc = self._lib.accbpg_fw_get_state(self._inst_h(i), *[_ptr(t) for t in self._fw_snaps[i]])
                if rc:
                    _lib.check(rc, "accbpg_fw_get_state")

    def fw_restore(self, i):
        """Instance i back to its last ``fw_snapshot`` (``accbpg_fw_set_state``: no probe is pending afterwards); the
        other instances stay as they are."""
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_fw_set_state(self._inst_h(i), *[_ptr(t) for t in self._fw_snaps[i]])
        _lib.check(rc, "accbpg_fw_set_state")

    def fw_run(self, away, eps, nsteps, active=None):
        """``nsteps`` iterations of the active instances decided on the device behind one synchronisation
        (``accbpg_dopt_batch_fw_run``).  ``eps``: a scalar or one per instance.  Returns a list of K entries: for an active
        instance the records of the iterations that ran (``_lib.FwStep`` with status != 3; they live in a buffer the
        next call overwrites), None for an inactive one.  A record with status 2 (pivot outside [0, n)) is returned,
        not raised: the replay reaches it in its turn and calls ``bad_pivot``."""
        mask, idx = self._mask(active)
        K, nsteps = self.K, int(nsteps)
        if self._fw_steps is None:
            self._fw_steps = (_lib.FwStep * (K * _lib.FW_RUN_MAX))()
        epsv = (C.c_double * K)(*np.broadcast_to(np.asarray(eps, dtype=np.float64), (K,)))
        nrun = (C.c_int * K)()
        steps = self._fw_steps
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_dopt_batch_fw_run(self._h, int(away), epsv, nsteps, mask, steps, nrun)
        if rc:
            if not (rc == _lib.ERR_ARG and any(nrun[i] > 0 and steps[i * nsteps + nrun[i] - 1].status == _lib.FW_BAD_PIVOT
                                               for i in idx)):
                _lib.check(rc, "accbpg_dopt_batch_fw_run")
            self._fw_bad_pivot = _lib.last_error()              # (names the instance; kept for bad_pivot)
        out = [None] * K
        for i in idx:
            out[i] = steps[i * nsteps:i * nsteps + nrun[i]]
        return out

    def bad_pivot(self):
        """The exception of the sequential solver's ``update`` with a pivot outside [0, n), with the message of the
        ``fw_run`` call that returned the status-2 record (it names the instance)."""
        raise ValueError("accbpg_fw_update: bad argument (%s)" % self._fw_bad_pivot)

    def fw_logdet_ring(self, depth, small_launches=2):
        """``accbpg_fw_logdet_ring`` on every instance handle."""
        with torch.cuda.device(self.device):
            for i in range(self.K):
                _lib.check(self._lib.accbpg_fw_logdet_ring(self._inst_h(i), int(depth), int(small_launches)),
                           "accbpg_fw_logdet_ring")

    def fw_logdet_snapshot(self, active=None):
        """``accbpg_fw_logdet_snapshot`` on the active instances' handles: each snapshots its H into its own ring and
        starts the side factorisation.  Returns, per instance, the value of the slot that came round (nan: none)."""
        _, idx = self._mask(active)
        out = [float("nan")] * self.K
        val = C.c_double(0.0)
        with torch.cuda.device(self.device):
            for i in idx:
                _lib.check(self._lib.accbpg_fw_logdet_snapshot(self._inst_h(i), C.byref(val)), "accbpg_fw_logdet_snapshot")
                out[i] = val.value
        return out

    def fw_logdet_flush(self, i):
        """The oldest side factorisation of instance i still in flight (``accbpg_fw_logdet_flush``)."""
        val = C.c_double(0.0)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.accbpg_fw_logdet_flush(self._inst_h(i), C.byref(val)), "accbpg_fw_logdet_flush")
        return val.value

    def fw_state(self, i):
        """(x, w, H) of instance i as device tensors (``accbpg_fw_get_state`` on its handle)."""
        x = torch.empty(self.n, dtype=torch.float64, device=self.device)
        w = torch.empty(self.n, dtype=torch.float64, device=self.device)
        H = torch.empty(self.m, self.m, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_fw_get_state(self._inst_h(i), _ptr(x), _ptr(w), _ptr(H))
        _lib.check(rc, "accbpg_fw_get_state")
        return x, w, H

    def fw_x(self, i, as_numpy=True):
        x = torch.empty(self.n, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.accbpg_fw_get_state(self._inst_h(i), _ptr(x), None, None)
        _lib.check(rc, "accbpg_fw_get_state")
        return from_dev(x, as_numpy)


def _finish_rows(batch, runs, running, active, result_x, Gr, Xn, X, Zn):
    """The end of an outer iteration of the accelerated batches: the restart and stop tests of the instances in
    ``running`` (the indices set in ``active``).  Returns the next Z: Zn, or from the first restart on a copy of it with
    the restarted rows of Xn.  An instance that stops is cleared in ``active`` and its row of Xn kept in ``result_x``.
    The runs share their options and their k, so one of them speaks for all on whether the inner products are needed."""
    dots = runs[running[0]].needs_dot()
    rest = batch.ls_terms(Gr, Xn, X, None, None, active)[:, 0] if dots else [None] * batch.K    # <g, x+ - x>
    Znext = Zn
    for i in running:
        restarted, stop = runs[i].finish(rest[i])
        if restarted:
            if Znext is Zn:
                Znext = Zn.clone()
            Znext[i] = Xn[i]
        if stop:
            active[i] = False
            result_x[i] = Xn[i].clone()
    return Znext


def _results(runs, result_x, X, as_numpy):
    """Per instance, its run's tuple around the x it stopped at (its row of X if it ran all iterations)."""
    return [run.result(from_dev(result_x[i] if result_x[i] is not None else X[i].clone(), as_numpy))
            for i, run in enumerate(runs)]


def ABPG_batch_steps(batch, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=False, restart=False, restart_rule='g',
                     overlap=True):
    """ABPG (accbpg/algorithms.py:94-180) on the K instances of a ``DOptimalBatch`` in lock-step: every oracle call,
    prox and vector pass covers all instances that are still running.  theta, the restart state and the stopping test
    are kept per instance exactly as the sequential solver keeps them; an instance that stops (D(z+,z) < epsilon)
    drops out of the later launches.  Yields k after every outer iteration; returns, per instance, ABPG's
    (x, F, G, T) -- bit-identical to ``ABPG(batch.instance(i), h, L, x0, ...)``.  With `overlap` (default) the values
    F[k] = f(x_i) run on a second stream beside the gradient evaluations at y_i, which do not depend on them."""
    K = batch.K
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    Z = X.clone()
    runs = [_ABPGRun(L, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule) for _ in range(K)]
    active = [True] * K
    result_x = [None] * K
    eps_prox = getattr(h, "eps", 1e-8)
    for k in range(maxitrs):
        if not any(active):
            break
        side = overlap and not getattr(batch, "_prof", False)                # (kernel timing keeps everything on one stream)
        ticket = batch.value_async(X, active) if side else None             # :135 (beside the gradients below)
        fx = None if side else batch.func_grad(X, 0, active)
        now = time.time() - t_start
        running = [i for i in range(K) if active[i]]
        for i in running:
            runs[i].begin(k)                                                # :142-145
        theta = [run.theta for run in runs]
        one_m = [1 - t for t in theta]
        Y = batch.axpby(one_m, X, theta, Z, active)                         # :147
        Gr = batch.func_grad(Y, 1, active)                                  # :148
        if side:
            fx = batch.value_wait(ticket)
            now = time.time() - t_start
        for i in running:
            runs[i].record(fx[i] + h.extra_Psi(None), now)
        Zn = batch.prox(Z, Gr, [run.prox_coef() for run in runs], eps_prox, active)    # :149
        Xn = batch.axpby(one_m, X, theta, Zn, active)                       # :150
        terms = batch.ls_terms(None, Xn, Y, Zn, Z, active)                  # :153-154
        for i in running:
            runs[i].divergences(terms[i, 1], terms[i, 2])                   # :155
        X, Z = Xn, _finish_rows(batch, runs, running, active, result_x, Gr, Xn, X, Zn)     # :165-174
        yield k
    return _results(runs, result_x, X, as_numpy)


def ABPG_batch(batch, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=False, restart=False, restart_rule='g',
               overlap=True):
    """Drain ``ABPG_batch_steps``: list of (x, F, G, T), one per instance."""
    return _drain(ABPG_batch_steps(batch, h, L, x0, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule, overlap))


def BPG_batch_steps(batch, h, L, x0, maxitrs, epsilon=1e-14, linesearch=True, ls_ratio=1.2):
    """BPG (accbpg/algorithms.py:11-72) on the K instances of a ``DOptimalBatch`` in lock-step per ORACLE PASS: one
    evaluation of (f, grad) at the iterates of all running instances, then one prox + one trial value per pass of the
    backtracking search, for the instances that are still searching.  L is carried per instance (divided by ls_ratio
    before each search, :51; multiplied after each failed test, :54); an instance stops when |F[k] - F[k-1]| <
    epsilon (:66) and drops out of the later launches.  Yields k after every outer iteration; returns, per instance,
    BPG's (x, F, Ls, T) -- bit-identical to ``BPG(batch.instance(i), h, L, x0, ...)``."""
    K, n = batch.K, batch.n
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    runs = [_BPGRun(L, maxitrs, epsilon, linesearch, ls_ratio) for _ in range(K)]
    active = [True] * K
    result_x = [None] * K
    eps_prox = getattr(h, "eps", 1e-8)
    for k in range(maxitrs):
        if not any(active):
            break
        fx, Gr = batch.func_grad(X, 2, active)                              # :46
        now = time.time() - t_start
        running = [i for i in range(K) if active[i]]
        for i in running:
            runs[i].begin(k, fx[i] + h.extra_Psi(None), now)                # :47, :51
        Xt = torch.empty(K, n, dtype=torch.float64, device=batch.device)    # rows are written by the passes that need them
        search = list(active) if linesearch else []
        while any(search):                                                  # one pass = one trial per searching instance
            batch.prox(X, Gr, [run.L for run in runs], eps_prox, search, out=Xt)    # :52 / :55
            terms = batch.ls_terms(Gr, Xt, X, None, None, search)           # <g, x+ - x>, D(x+, x)
            ft = batch.func_grad(Xt, 0, search)                             # :53
            for i in running:
                if search[i] and runs[i].accepts(ft[i], fx[i], terms[i, 0], terms[i, 1]):    # :53-54
                    search[i] = False
        if not linesearch:
            batch.prox(X, Gr, [run.L for run in runs], eps_prox, active, out=Xt)    # :58
        for i in running:
            if runs[i].finish():                                            # :66
                active[i] = False
                result_x[i] = Xt[i].clone()
        X = Xt
        yield k
    return _results(runs, result_x, X, as_numpy)


def BPG_batch(batch, h, L, x0, maxitrs, epsilon=1e-14, linesearch=True, ls_ratio=1.2):
    """Drain ``BPG_batch_steps``: list of (x, F, Ls, T), one per instance."""
    return _drain(BPG_batch_steps(batch, h, L, x0, maxitrs, epsilon, linesearch, ls_ratio))


def solve_instances(make_problem, num_instances, solver, world=1, rank=0, threads=None, concurrent=True,
                    group=None, **solver_kwargs):
    """BASELINE config 4 end to end: deal `num_instances` independent problems to the ranks
    (``split_instances``: round-robin, so instances that stop early spread out), solve this rank's share
    concurrently on its GPU, and gather every instance's result on every rank, in instance order.

    make_problem(i) -> (f, h, L, x0) builds instance i (only called for the instances of this rank);
    solver(f, h, L, x0, **solver_kwargs) is any solver of this package.  There is no data-path collective:
    the only communication is the result gather (torch.distributed all_gather_object over the process
    group that is already up -- RCCL ranks use their gloo/object path for this small host payload).
    `concurrent=False` runs the share sequentially on the calling thread (no streams; what the CPU tests of
    the dealing and gathering use with stand-in problems)."""
    from .sharded import split_instances
    mine = split_instances(num_instances, world, rank)
    problems = [make_problem(i) for i in mine]
    if concurrent:
        results = solve_batch(problems, solver, threads=threads, **solver_kwargs)
    else:
        results = [solver(*prob, **solver_kwargs) for prob in problems]
    local = {i: _to_host(res) for i, res in zip(mine, results)}
    if world > 1:
        import torch.distributed as dist
        shares = [None] * world
        dist.all_gather_object(shares, local, group=group)
        merged = {}
        for share in shares:
            merged.update(share)
    else:
        merged = local
    return [merged[i] for i in range(num_instances)]


def _to_host(result):
    """Solver results as host data (NumPy / floats) so that they can be shipped between ranks."""
    if isinstance(result, torch.Tensor):
        return result.detach().cpu().numpy()
    if isinstance(result, (tuple, list)):
        return type(result)(_to_host(r) for r in result)
    return result


def solve_batch(problems, solver, threads=None, **solver_kwargs):
    """Run ``solver(f, h, L, x0, **solver_kwargs)`` for every (f, h, L, x0) in `problems`
    concurrently; returns the list of results in order.  `solver` is any of BPG / ABPG /
    ABPG_gain (or D_opt_FW-style callables taking the same leading arguments)."""
    if not problems:
        return []
    threads = min(len(problems), threads or 8)
    device = problems[0][0].device

    def run(prob):
        f, h, L, x0 = prob
        stream = torch.cuda.Stream(device=device)
        with torch.cuda.device(device), torch.cuda.stream(stream):
            out = solver(f, h, L, x0, **solver_kwargs)
            stream.synchronize()
        return out

    with ThreadPoolExecutor(max_workers=threads) as pool:
        return list(pool.map(run, problems))


class BatchStepper:
    """Step generators of several instances advanced concurrently (used by bench.py): every call
    of ``step()`` advances each instance by one outer iteration."""

    def __init__(self, make_generators, device, threads=None):
        self.device = device
        self.n = len(make_generators)
        self.threads = min(self.n, threads or 8)
        self._gens = [None] * self.n
        self._streams = [torch.cuda.Stream(device=device) for _ in range(self.n)]
        self._pool = ThreadPoolExecutor(max_workers=self.threads)
        self._make = make_generators

    def _advance(self, idx, count):
        with torch.cuda.device(self.device), torch.cuda.stream(self._streams[idx]):
            if self._gens[idx] is None:
                self._gens[idx] = self._make[idx]()
            for _ in range(count):
                next(self._gens[idx])
            self._streams[idx].synchronize()
        return idx

    def step(self, count=1):
        list(self._pool.map(lambda i: self._advance(i, count), range(self.n)))

    def close(self):
        self._pool.shutdown()


def ABPG_gain_batch_steps(batch, h, L, x0, gamma, maxitrs, epsilon=1e-14, G0=1, ls_inc=1.2, ls_dec=1.2, theta_eq=True,
                          checkdiv=False, restart=False, restart_rule='g', overlap=True):
    """ABPG_gain (accbpg/algorithms.py:295-420) on the K instances of a ``DOptimalBatch`` in lock-step per ORACLE
    PASS: every gradient evaluation, prox, vector pass and trial value covers the instances that need it.  The line
    search is per instance -- each keeps its own gain, theta and retry count on the host; after a pass the instances
    whose test failed raise their gain and take part in the next pass, the others have accepted their point and
    wait (their rows are not touched again in this outer iteration).  Yields k after every outer iteration; returns,
    per instance, ABPG_gain's (x, F, Gain, Gdiv, Gavg, T) -- bit-identical to ``ABPG_gain(batch.instance(i), ...)``."""
    K, n = batch.K, batch.n
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    Z = X.clone()
    runs = [_GainRun(L, gamma, maxitrs, epsilon, G0, ls_inc, ls_dec, theta_eq, checkdiv, restart, restart_rule)
            for _ in range(K)]
    active = [True] * K
    result_x = [None] * K
    eps_prox = getattr(h, "eps", 1e-8)
    new = lambda: torch.empty(K, n, dtype=torch.float64, device=batch.device)
    for k in range(maxitrs):
        if not any(active):
            break
        side = overlap and not getattr(batch, "_prof", False)                # (kernel timing keeps everything on one stream)
        ticket = batch.value_async(X, active) if side else None             # :347 (beside the first gradients below)
        fx = None if side else batch.func_grad(X, 0, active)
        now = time.time() - t_start
        running = [i for i in range(K) if active[i]]
        for i in running:
            runs[i].begin(k)                                                # :358
        search = list(active)
        Y, Gr, Zt, Xt = new(), new(), new(), new()                          # rows are written by the passes that need them
        first_pass = True
        while any(search):                                                  # :361, one pass = one trial per searching instance
            theta = [run.trial() if search[i] else run.theta for i, run in enumerate(runs)]    # :362-367
            one_m = [1 - t for t in theta]
            batch.axpby(one_m, X, theta, Z, search, out=Y)                  # :369
            fy, _ = batch.func_grad(Y, 2, search, out=Gr)                   # :371
            if first_pass:
                if side:
                    fx = batch.value_wait(ticket)
                    now = time.time() - t_start
                for i in running:
                    runs[i].record(fx[i] + h.extra_Psi(None), now)          # :348
                first_pass = False
            batch.prox(Z, Gr, [run.prox_coef() for run in runs], eps_prox, search, out=Zt)   # :373
            batch.axpby(one_m, X, theta, Zt, search, out=Xt)                # :374
            terms = batch.ls_terms(Gr, Xt, Y, Zt, Z, search)                # :377-378 and the dot of :387
            need_value = [False] * K
            for i in running:
                if search[i]:
                    verdict = runs[i].divergences(*terms[i])                # :379-385
                    need_value[i] = verdict == NEEDS_VALUE
                    search[i] = verdict in (NEEDS_VALUE, RETRY)
            if any(need_value):
                ft = batch.func_grad(Xt, 0, need_value)                     # :387
                for i in running:
                    if need_value[i]:
                        search[i] = runs[i].value(ft[i], fy[i]) == RETRY
        X, Z = Xt, _finish_rows(batch, runs, running, active, result_x, Gr, Xt, X, Zt)     # :395-412
        yield k
    return _results(runs, result_x, X, as_numpy)


def ABPG_gain_batch(batch, h, L, x0, gamma, maxitrs, **kwargs):
    """Drain ``ABPG_gain_batch_steps``: list of (x, F, Gain, Gdiv, Gavg, T), one per instance."""
    return _drain(ABPG_gain_batch_steps(batch, h, L, x0, gamma, maxitrs, **kwargs))


def ABPG_expo_batch_steps(batch, h, L, x0, gamma0, maxitrs, epsilon=1e-14, delta=0.2, theta_eq=True, checkdiv=False,
                          Gmargin=10, restart=False, restart_rule='g', overlap=True):
    """ABPG_expo (accbpg/algorithms.py:183-292) on the K instances of a ``DOptimalBatch`` in lock-step per ORACLE
    PASS: one evaluation of (f, grad) at y for all running instances per outer iteration (:245), then passes of prox,
    vector combination, divergences and -- unless `checkdiv` -- a trial value for the instances that are still lowering
    their exponent; the others have accepted their point and their rows are not touched again in this outer iteration.
    The exponent, theta, the restart state and the stopping test are kept per instance on the host.  Yields k after
    every outer iteration; returns, per instance, ABPG_expo's (x, F, Gamma, G, T) -- bit-identical to
    ``ABPG_expo(batch.instance(i), ...)``.  Where the value test accepted x+ it evaluated f there, and that number is
    F[k+1] (the same kernel on the same vector: the same bits), so F[k] is evaluated only for the instances that have none
    -- at k = 0 and with `checkdiv`; with `overlap` (default) on a second stream beside the evaluations at y_i."""
    K, n = batch.K, batch.n
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    Z = X.clone()
    runs = [_ExpoRun(L, gamma0, maxitrs, epsilon, delta, theta_eq, checkdiv, Gmargin, restart, restart_rule)
            for _ in range(K)]
    active = [True] * K
    result_x = [None] * K
    eps_prox = getattr(h, "eps", 1e-8)
    new = lambda: torch.empty(K, n, dtype=torch.float64, device=batch.device)
    carried = [None] * K                        # f at the rows of X that the accepting value test of the last iteration left
    for k in range(maxitrs):
        if not any(active):
            break
        due = [active[i] and carried[i] is None for i in range(K)]
        side = overlap and any(due) and not getattr(batch, "_prof", False)   # (kernel timing keeps everything on one stream)
        ticket = batch.value_async(X, due) if side else None                # :231 (beside the evaluation below)
        fx = batch.func_grad(X, 0, due) if any(due) and not side else None
        now = time.time() - t_start
        running = [i for i in range(K) if active[i]]
        for i in running:
            runs[i].begin(k)                                                # :238-241
        theta = [run.theta for run in runs]
        one_m = [1 - t for t in theta]
        Y = batch.axpby(one_m, X, theta, Z, active)                         # :243
        fy, Gr = batch.func_grad(Y, 2, active)                              # :245
        if side:
            fx = batch.value_wait(ticket)
            now = time.time() - t_start
        for i in running:
            runs[i].record((fx[i] if due[i] else carried[i]) + h.extra_Psi(None), now)      # :232
        carried = [None] * K
        search = list(active)
        Zt, Xt = new(), new()                                               # rows are written by the passes that need them
        while any(search):                                                  # :248, one pass = one trial per searching instance
            batch.prox(Z, Gr, [run.prox_coef() for run in runs], eps_prox, search, out=Zt)   # :249
            batch.axpby(one_m, X, theta, Zt, search, out=Xt)                # :250
            terms = batch.ls_terms(Gr, Xt, Y, Zt, Z, search)                # :253-254 and the dot of :260
            need_value = [False] * K
            for i in running:
                if search[i]:
                    verdict = runs[i].divergences(*terms[i])                # :255-258
                    need_value[i] = verdict == NEEDS_VALUE
                    search[i] = verdict in (NEEDS_VALUE, RETRY)
            if any(need_value):
                ft = batch.func_grad(Xt, 0, need_value)                     # :260
                for i in running:
                    if need_value[i]:
                        search[i] = runs[i].value(ft[i], fy[i]) == RETRY    # :262-265
                        carried[i] = None if search[i] else ft[i]
        X, Z = Xt, _finish_rows(batch, runs, running, active, result_x, Gr, Xt, X, Zt)     # :267-285
        yield k
    return _results(runs, result_x, X, as_numpy)


def ABPG_expo_batch(batch, h, L, x0, gamma0, maxitrs, **kwargs):
    """Drain ``ABPG_expo_batch_steps``: list of (x, F, Gamma, G, T), one per instance."""
    return _drain(ABPG_expo_batch_steps(batch, h, L, x0, gamma0, maxitrs, **kwargs))


def ABDA_batch_steps(batch, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=True, overlap=True):
    """ABDA (accbpg/algorithms.py:423-514) on the K instances of a ``DOptimalBatch`` in lock-step: per outer iteration
    one vector combination for y, one gradient call, one ``avg_prox`` -- the weighted gradient average, its quotient by
    the sum of the weights and the prox of that in a single launch --, one combination for x and one pass for the
    divergences, each over all instances that are still running.  The averages ping-pong between two K x n buffers.
    theta, the sum of the weights and the stopping test are kept per instance on the host.  Yields k after every outer
    iteration; returns, per instance, ABDA's (x, F, G, T) -- bit-identical to ``ABDA(batch.instance(i), ...)``.  With
    `overlap` (default) the values F[k] = f(x_i) run on a second stream beside the gradient evaluations at y_i."""
    K, n = batch.K, batch.n
    t_start = time.time()
    X, as_numpy = batch.fw_rows(x0)
    Z = X.clone()
    runs = [_ABDARun(L, gamma, maxitrs, epsilon, theta_eq) for _ in range(K)]
    active = [True] * K
    result_x = [None] * K
    eps_prox = getattr(h, "eps", 1e-8)
    Gavg = torch.zeros(K, n, dtype=torch.float64, device=batch.device)
    Gavg_next = torch.empty(K, n, dtype=torch.float64, device=batch.device)
    for k in range(maxitrs):
        if not any(active):
            break
        side = overlap and not getattr(batch, "_prof", False)                # (kernel timing keeps everything on one stream)
        ticket = batch.value_async(X, active) if side else None             # :465 (beside the gradients below)
        fx = None if side else batch.func_grad(X, 0, active)
        now = time.time() - t_start
        running = [i for i in range(K) if active[i]]
        for i in running:
            runs[i].begin(k)                                                # :472-475
        theta = [run.theta for run in runs]
        one_m = [1 - t for t in theta]
        Y = batch.axpby(one_m, X, theta, Z, active)                         # :477
        Gr = batch.func_grad(Y, 1, active)                                  # :478
        if side:
            fx = batch.value_wait(ticket)
            now = time.time() - t_start
        for i in running:
            runs[i].record(fx[i] + h.extra_Psi(None), now)                  # :466
        wgt, csum, Lc = zip(*[run.weight() if active[i] else (0.0, 1.0, 1.0) for i, run in enumerate(runs)])   # :480
        _, Zn = batch.avg_prox(Gavg, Gr, wgt, csum, Lc, eps_prox, active, out_avg=Gavg_next)     # :479, :481
        Gavg, Gavg_next = Gavg_next, Gavg                   # (a stopped instance's row goes stale: it is not read again)
        Xn = batch.axpby(one_m, X, theta, Zn, active)                       # :482
        terms = batch.ls_terms(None, Xn, Y, Zn, Z, active)                  # :485-486
        for i in running:
            runs[i].divergences(terms[i, 1], terms[i, 2])                   # :491
        X, Z = Xn, _finish_rows(batch, runs, running, active, result_x, None, Xn, X, Zn)    # :508
        yield k
    return _results(runs, result_x, X, as_numpy)


def ABDA_batch(batch, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=True, overlap=True):
    """Drain ``ABDA_batch_steps``: list of (x, F, G, T), one per instance."""
    return _drain(ABDA_batch_steps(batch, h, L, x0, gamma, maxitrs, epsilon, theta_eq, overlap))
