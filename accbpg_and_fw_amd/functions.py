"""Device-backed mirror of the f / h object protocol of the reference
(accbpg/functions.py:10-59, 199-271, 326-356).

Same class names, method names, argument meaning and exceptions, so the
reference's own solver loops (and this package's) can call them unchanged.
Vectors may be NumPy arrays (copied to the GPU and results copied back, for
drop-in use from NumPy drivers) or fp64 CUDA tensors (kept on the device, the
fast path used by this package's solvers).  All arithmetic runs in
libaccbpg_hip.so; torch only owns memory and streams.
"""
from __future__ import annotations

import ctypes as C
import threading

import numpy as np
import torch

from . import _lib


# ------------------------------------------------------------------ helpers
def _device():
    if not torch.cuda.is_available():
        raise RuntimeError("accbpg_and_fw_amd needs an AMD GPU (torch.cuda is not available); "
                           "there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def to_dev(a):
    """-> (fp64 contiguous CUDA tensor, came_from_numpy)."""
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float64:
            a = a.to(torch.float64)
        if not a.is_cuda:
            return a.to(_device()).contiguous(), False
        return a.contiguous(), False
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    return torch.from_numpy(arr).to(_device()), True


def from_dev(t, as_numpy):
    return t.cpu().numpy() if as_numpy else t


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


class _Workspace:
    """Scratch for the length-n kernels, one per (host thread, device, n).  Kept per thread (it goes away with
    the thread, so generations of pool workers do not pile up) and bounded per thread: the least recently
    used size is dropped beyond `_KEEP` entries."""
    _local = threading.local()
    _KEEP = 8

    @classmethod
    def get(cls, n, device):
        cache = getattr(cls._local, "cache", None)
        if cache is None:
            cache = cls._local.cache = {}
        key = (device.index, int(n))
        ws = cache.pop(key, None)
        if ws is None:
            size = _lib.load().accbpg_vec_workspace_doubles(int(n))
            ws = torch.empty(size, dtype=torch.float64, device=device)
            while len(cache) >= cls._KEEP:
                cache.pop(next(iter(cache)))
        cache[key] = ws                      # most recently used last
        return ws


_WS = object()      # in the arguments of _call: the pointer to the workspace of the reference tensor's size


def _call(name, ref, *args, assert_msg=None):
    """The C entry `name` on ref's device: args (with _WS filled in) and the current stream, then the status check."""
    with torch.cuda.device(ref.device):
        args = [_ptr(_Workspace.get(ref.numel(), ref.device)) if a is _WS else a for a in args]
        rc = getattr(_lib.load(), name)(*args, _stream())
    _lib.check(rc, name, assert_msg)


# ------------------------------------------------------------------ f
class RSmoothFunction:
    """Relatively-smooth function protocol (accbpg/functions.py:10-24)."""

    def __call__(self, x):
        assert 0, "RSmoothFunction: __call__(x) is not defined"

    def gradient(self, x):
        assert 0, "RSmoothFunction: gradient(x) is not defined"

    def func_grad(self, x, flag):
        assert 0, "RSmoothFunction: func_grad(x, flag) is not defined"


class DOptimalObj(RSmoothFunction):
    """f(x) = -log det(H diag(x) H^T), H m x n with m < n  (accbpg/functions.py:27-59).

    ``H`` may be a NumPy array (copied to the GPU once) or an fp64 CUDA tensor
    (borrowed).  ``self.H``, ``self.m``, ``self.n`` stay readable as in the
    reference (callers use ``f.H``)."""

    def __init__(self, H, _shard=False, _borrowed=None):
        self.H = H
        self.m = H.shape[0]
        self.n = H.shape[1]
        # a column shard of a larger instance may have fewer columns than rows
        assert _shard or self.m < self.n, "DOptimalObj: need m < n"
        self._V, _ = to_dev(H)
        self._is_shard = bool(_shard)
        lib = _lib.load()
        if _borrowed is not None:
            # one instance of a DOptimalBatch: the handle belongs to the batch (kept alive through _owner)
            h, self._owner = _borrowed
            self._owned = False
        else:
            h = C.c_void_p()
            with torch.cuda.device(self._V.device):
                rc = lib.accbpg_dopt_create(_ptr(self._V), self.m, self.n, self._V.stride(0), _stream(), C.byref(h),
                                            1 if _shard else 0)
            _lib.check(rc, "accbpg_dopt_create")
            self._owned = True
        self._h = h
        self._lib = lib
        self.calls = {"value": 0, "grad": 0}
        # F[k] = f(x) of the accelerated solvers runs beside the gradient evaluation (see overlap_values())
        self._overlap = True
        self._spec = False
        self.spec_unused = 0
        self._prof = False
        # opt-in reuse of resident Gram matrices through linearity (see linear_gram())
        self._lin = False
        self._gcache = []           # [(vector tensor, Gram tensor, age)], most recent last
        self._gcache_cap = 5
        self._lin_refresh = 50
        self.gram_launches = 0
        self.gram_combos = 0
        self.value_hits = 0
        self._reuse = True
        # ABPG_gain's line-search trials go through accbpg_dopt_burg_trial (see one_wait_trials())
        self._one_wait = True
        self.one_wait_trials_run = 0

    def __del__(self):
        for name in ("_h", "_h2"):
            h = getattr(self, name, None)
            if name == "_h" and not getattr(self, "_owned", True):
                continue
            if h:
                try:
                    self._lib.accbpg_dopt_destroy(h)
                except Exception:
                    pass
                setattr(self, name, None)

    # ---- a value evaluation that runs beside other work (second handle, second stream) ----
    def overlap_values(self, enable=True):
        """The accelerated solvers evaluate F[k] = f(x) on a side stream beside the gradient evaluation at y,
        which does not depend on it (accbpg/algorithms.py:135/148, :347/371): the latency-bound factorisation
        of one evaluation runs under the MFMA-bound products of the other.  Identical kernels and bit-identical
        results; on by default, ``overlap_values(False)`` puts both evaluations on the solver's stream."""
        self._overlap = bool(enable)
        return self

    def value_async(self, x):
        """Start f(x) on a side stream and return a ticket for ``value_wait``.  The accelerated
        solvers use it for F[k] = f(x), which the gradient evaluation at y does not depend on, so the
        latency-bound factorisation of one evaluation runs under the MFMA-bound products of the
        other.  Same kernels, same results as ``f(x)``."""
        assert x.numel() == self.n, "DOptimalObj: x.size not equal to n"
        self._side_handle()
        with torch.cuda.device(self._V.device):
            self._side.wait_stream(torch.cuda.current_stream())          # x is produced on the caller's stream
            rc = self._lib.accbpg_dopt_func_grad_begin(self._h2, _ptr(x), 0, None)
        _lib.check(rc, "accbpg_dopt_func_grad_begin")
        return x                                                          # the ticket keeps x alive

    def value_wait(self, ticket):
        fval = C.c_double(0.0)
        with torch.cuda.device(self._V.device):
            rc = self._lib.accbpg_dopt_func_grad_end(self._h2, C.byref(fval))
        _lib.check(rc, "accbpg_dopt_func_grad_end", "DOptimalObj: x needs to be nonnegative")
        self.calls["value"] += 1
        self._memo_put(ticket, fval.value)                      # (the ticket is the evaluated tensor)
        return fval.value

    # ---- a gradient evaluation started ahead of the decision that may need it (second handle, second stream) ----
    def speculate(self, enable=True):
        """Opt-in.  ABPG_gain's gain is cut before every search (accbpg/algorithms.py:358) and raised again on
        failure (:390), so once it has settled the search retries about once per iteration.  With this switch on the
        solver starts the gradient evaluation of the NEXT trial point -- which depends on host scalars and the
        previous iterates only -- on the side stream beside the value test of the current one, whenever the previous
        iteration needed that retry too; a trial that passes leaves the extra evaluation unused.  Every evaluation
        that IS used is the one the sequential loop would have made: results are bit-identical
        (test_gradients_started_ahead_change_nothing).  Off by default: the retry counts are irregular (0,1,1,2,...
        around an average of one), about a quarter of the evaluations started ahead go unused, and an unused one
        costs more than a used one saves -- measured 50.5 -> 47.7 it/s at (2048,32768), 562 -> 578 at (512,8192)."""
        self._spec = bool(enable)
        return self

    # ---- f at a vector object that was evaluated a moment ago (extension; off unless enabled) ----
    def memoize_values(self, enable=True):
        """Opt-in.  The reference evaluates f at the accepted line-search point twice: in the test that accepts it
        (accbpg/algorithms.py:387) and again as F[k+1] = f(x) at the top of the next iteration (:347).  With this switch
        on, f(x) at the very tensor object whose value was the last one computed is answered from that value instead of
        a second Gram product and factorisation -- the same number to the bit (the kernels are deterministic), one
        value evaluation fewer per ABPG_gain iteration (3 -> 2 in the steady state).  Off by default because it is not
        how the reference spends its time; bench.py reports it apart (`--memo-values`)."""
        self._memo_on = bool(enable)
        self._memo = None
        return self

    # ---- f at a device vector whose value the library computed a moment ago (on by default) ----
    def reuse_values(self, enable=True):
        """ABPG_gain evaluates f at the accepted line-search point twice (accbpg/algorithms.py:387, then F[k+1] = f(x)
        at :347).  The library keeps the last value-only evaluation of each handle -- device address, a copy of x, f --
        and answers a value evaluation at the same address with the same 64-bit content from it: no Gram product, no
        factorisation, the same number to the bit (accbpg_dopt_value_reuse in include/accbpg_hip.h).  On by default;
        ``reuse_values(False)`` makes every evaluation run.  ``calls["value"]`` counts the values the solver asked
        for either way, ``values_reused`` those that were answered."""
        self._reuse = bool(enable)
        for h in self._handles():
            self._lib.accbpg_dopt_value_reuse(h, 1 if enable else 0)
        return self

    @property
    def values_reused(self):
        total = 0
        for h in self._handles():
            cmp_, ans = C.c_int64(0), C.c_int64(0)
            self._lib.accbpg_dopt_value_reuse_stats(h, C.byref(cmp_), C.byref(ans))
            total += ans.value
        return total

    # ---- a whole line-search trial of ABPG_gain enqueued at once and waited for once (on by default) ----
    def one_wait_trials(self, enable=True):
        """A trial of ABPG_gain's line search is y, func_grad(y), the prox, x, the three line-search terms and f(x)
        (accbpg/algorithms.py:369-387).  None of the intermediate results decides what is launched next, so with a
        BurgEntropySimplex kernel, device iterates and ``checkdiv`` off the solver enqueues the whole trial -- and the
        lookup that answers F[k] from the value record (``reuse_values``) -- through ``accbpg_dopt_burg_trial`` and
        waits once instead of five times.  Same launches, bit-identical results, same ``calls`` and ``values_reused``; a
        trial that is not clean (a flag of any stage) commits nothing and is run again through the stepwise calls,
        which raise what the stepwise loop raises.  On by default; ``one_wait_trials(False)`` gives the stepwise loop.
        Not used with ``linear_gram``, ``speculate`` or ``memoize_values``, on a shard or in a batch, or when
        ``func_grad`` -- or a method of the Burg simplex kernel -- has been wrapped or overridden (the solver then
        calls it, as before).  After a replay in an iteration whose F[k] rode in the trial the record is gone and F[k]
        is evaluated in full: ``values_reused`` is then one less than the stepwise loop's.
        ``one_wait_trials_run`` counts the trials that went through the entry."""
        self._one_wait = bool(enable)
        return self

    def _one_wait_ok(self):
        # (an objective whose func_grad was wrapped on the instance or overridden in a subclass -- instrumentation, a
        # delay, a counter -- is evaluated through that func_grad, which a native trial would pass by)
        if "func_grad" in self.__dict__ or type(self).func_grad is not DOptimalObj.func_grad:
            return False
        return self._one_wait and self._owned and not self._is_shard and not (self._lin or self._spec or getattr(self, "_memo_on", False))

    def value_recorded(self, x):
        """True when a value evaluation at the device vector x would find a record at its address (the host-side
        part of the lookup of ``reuse_values``; the contents are compared on the device)."""
        return bool(self._lib.accbpg_dopt_value_recorded(self._h, _ptr(x)))

    def trial(self, x_prev, z_prev, theta, L, eps, want_fk):
        """One trial through accbpg_dopt_burg_trial on the current stream.  None for a trial that has to be replayed
        stepwise; else (y, g, z, x, TrialOut).  Counts the evaluations of a clean trial as the stepwise calls would,
        except f(x), which the caller counts when it uses it."""
        dev = self._V.device
        y, g, z, x = (torch.empty(self.n, dtype=torch.float64, device=dev) for _ in range(4))
        out = _lib.TrialOut()
        with torch.cuda.device(dev):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_burg_trial(self._h, _ptr(x_prev), _ptr(z_prev), float(theta), float(L),
                                                  float(eps), 1 if want_fk else 0, _ptr(y), _ptr(g), _ptr(z), _ptr(x),
                                                  _ptr(_Workspace.get(self.n, dev)), C.byref(out))
        self.one_wait_trials_run += 1
        if rc == _lib.TRIAL_REPLAY:
            return None
        _lib.check(rc, "accbpg_dopt_burg_trial")
        self.calls["grad"] += 1
        if out.fk_answered:
            self.calls["value"] += 1
        return y, g, z, x, out

    def _memo_get(self, x):
        memo = getattr(self, "_memo", None)
        if getattr(self, "_memo_on", False) and memo is not None and memo[0] is x and memo[1] == x._version:
            self.value_hits += 1
            self.calls["value"] += 1
            return memo[2]
        return None

    def _memo_put(self, x, value):
        if getattr(self, "_memo_on", False) and isinstance(x, torch.Tensor):
            self._memo = (x, x._version, value)                 # (holds x: its storage cannot be reused meanwhile)

    def _side_handle(self):
        if getattr(self, "_h2", None) is None:
            h2 = C.c_void_p()
            with torch.cuda.device(self._V.device):
                self._side = torch.cuda.Stream(device=self._V.device)
                rc = self._lib.accbpg_dopt_create(_ptr(self._V), self.m, self.n, self._V.stride(0),
                                                  C.c_void_p(self._side.cuda_stream), C.byref(h2), 1)
            _lib.check(rc, "accbpg_dopt_create")
            self._h2 = h2
            # its evaluations run beside the gradient evaluation of the solver's own stream: a launch per block
            # column leaves that stream its compute units (bit-identical results)
            self._lib.accbpg_dopt_factor_in_small_launches(h2, 2)
            # f(x) of the accepting test runs on one handle, F[k+1] = f(x) on the other: each may answer from the
            # other's record (reuse_values)
            self._lib.accbpg_dopt_value_reuse(h2, 1 if self._reuse else 0)
            _lib.check(self._lib.accbpg_dopt_value_peer(h2, self._h), "accbpg_dopt_value_peer")
            _lib.check(self._lib.accbpg_dopt_value_peer(self._h, h2), "accbpg_dopt_value_peer")
            if self._prof:
                self._lib.accbpg_dopt_profile_enable(self._h2, 1)
        return self._h2

    def grad_async(self, y):
        """Start func_grad(y, 2) on the side stream; returns a ticket for ``grad_wait`` / ``grad_drop``."""
        h2 = self._side_handle()
        g = torch.empty(self.n, dtype=torch.float64, device=self._V.device)
        with torch.cuda.device(self._V.device):
            self._side.wait_stream(torch.cuda.current_stream())          # y is produced on the caller's stream
            y.record_stream(self._side)
            g.record_stream(self._side)
            rc = self._lib.accbpg_dopt_func_grad_begin(h2, _ptr(y), 2, _ptr(g))
        _lib.check(rc, "accbpg_dopt_func_grad_begin")
        return (y, g)

    def grad_wait(self, ticket):
        y, g = ticket
        fval = C.c_double(0.0)
        with torch.cuda.device(self._V.device):
            rc = self._lib.accbpg_dopt_func_grad_end(self._h2, C.byref(fval))
            torch.cuda.current_stream().wait_stream(self._side)          # g is consumed on the caller's stream
        _lib.check(rc, "accbpg_dopt_func_grad_end", "DOptimalObj: x needs to be nonnegative")
        self.calls["grad"] += 1
        return fval.value, g

    def grad_drop(self, ticket):
        """The trial passed: the evaluation started ahead is not needed (it finishes on its own; its buffers are
        returned to the allocator only behind it)."""
        self.spec_unused += 1

    def value_lead_seconds(self):
        """How long before the last evaluation on the solver's stream the last side-stream value was known
        (0 when it was known later): what the solvers subtract so that T[k] is the moment F[k] existed."""
        ms = C.c_double(0.0)
        rc = self._lib.accbpg_dopt_eval_gap_ms(self._h2, self._h, C.byref(ms))
        return max(0.0, ms.value * 1e-3) if rc == _lib.OK else 0.0

    @property
    def device(self):
        return self._V.device

    @property
    def V_dev(self):
        return self._V

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def func_grad(self, x, flag=2):
        """flag=0: function, flag=1: gradient, flag=2: function & gradient."""
        assert (x.numel() if isinstance(x, torch.Tensor) else x.size) == self.n, \
            "DOptimalObj: x.size not equal to n"
        if flag == 0 and isinstance(x, torch.Tensor):
            hit = self._memo_get(x)
            if hit is not None:
                return hit
        xd, was_np = to_dev(x)
        fval = C.c_double(0.0)
        g = None
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            if flag != 0:
                g = torch.empty(self.n, dtype=torch.float64, device=self._V.device)
            rc = self._lib.accbpg_dopt_func_grad(self._h, _ptr(xd), int(flag), C.byref(fval), _ptr(g))
        _lib.check(rc, "accbpg_dopt_func_grad", "DOptimalObj: x needs to be nonnegative")
        self.calls["value" if flag == 0 else "grad"] += 1
        if flag == 0:
            self._memo_put(x, fval.value)
            return fval.value
        g = from_dev(g, was_np)
        return g if flag == 1 else (fval.value, g)

    # ---- Gram-matrix reuse through linearity (extension; off unless enabled) ----
    def linear_gram(self, enable=True, refresh=50, capacity=5):
        """V diag(x) V^T is linear in x.  When enabled, the accelerated solvers of this package
        tell the objective that a point is a*x1 + b*x2 (``func_grad_combo``); if the Gram matrices at
        x1 and x2 are still resident, the O(m^2 n) Gram launch is replaced by an O(m^2) combination.
        A chain of combinations is cut every `refresh` links by a direct evaluation so rounding does
        not accumulate.  Results agree with direct evaluation to rounding (tests pin 1e-12)."""
        self._lin = bool(enable)
        self._lin_refresh = int(refresh)
        self._gcache_cap = int(capacity)
        self._gcache = []
        return self

    def _gram_lookup(self, vec):
        for idx, ent in enumerate(self._gcache):
            if ent[0] is vec:
                self._gcache.append(self._gcache.pop(idx))      # least recently used first
                return ent
        return None

    def ensure_gram(self, x):
        """Make the Gram matrix at the (fresh) device vector x resident."""
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            if self._gram_lookup(x) is None:
                self._gram_direct(x)

    def _gram_store(self, vec, gram, age):
        self._gcache = [e for e in self._gcache if e[0] is not vec]
        self._gcache.append([vec, gram, age, None])             # [vector, Gram, chain length, f value]
        if len(self._gcache) > self._gcache_cap:
            self._gcache.pop(0)

    def _gram_buffer(self):
        # recycle the buffer that is about to fall out of the cache
        if len(self._gcache) >= self._gcache_cap:
            return self._gcache.pop(0)[1]
        return torch.empty(self.m, self.m, dtype=torch.float64, device=self._V.device)

    def _gram_direct(self, xd):
        gram = self._gram_buffer()
        rc = self._lib.accbpg_dopt_gram(self._h, _ptr(xd), _ptr(gram))
        _lib.check(rc, "accbpg_dopt_gram")
        self.gram_launches += 1
        self._gram_store(xd, gram, 0)
        return gram

    def func_grad_combo(self, x, combo, flag=2):
        """func_grad(x, flag) where the caller states x = a*x1 + b*x2 (combo = (a, x1, b, x2)), or
        combo=None for a fresh point.  Device tensors only."""
        assert x.numel() == self.n, "DOptimalObj: x.size not equal to n"
        fval = C.c_double(0.0)
        g = None
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            ent = self._gram_lookup(x)
            if ent is not None:
                gram = ent[1]
            else:
                gram = None
                if combo is not None:
                    a, x1, b, x2 = combo
                    e1, e2 = self._gram_lookup(x1), self._gram_lookup(x2)
                    if e1 is not None and e2 is not None and max(e1[2], e2[2]) < self._lin_refresh:
                        g1, g2, age = e1[1], e2[1], max(e1[2], e2[2]) + 1   # read before a buffer is recycled
                        gram = self._gram_buffer()
                        rc = self._lib.accbpg_dopt_gram_lincomb(self._h, float(a), _ptr(g1), float(b), _ptr(g2),
                                                                _ptr(gram))
                        _lib.check(rc, "accbpg_dopt_gram_lincomb")
                        self.gram_combos += 1
                        self._gram_store(x, gram, age)
                if gram is None:
                    gram = self._gram_direct(x)
            ent = self._gram_lookup(x)
            if flag == 0 and ent is not None and ent[3] is not None:
                # the same (immutable) vector object was already evaluated: the solvers test f(x+) in
                # the line search and record F[k+1] = f(x+) at the top of the next iteration
                self.calls["value"] += 1
                self.value_hits += 1
                return ent[3]
            if flag != 0:
                g = torch.empty(self.n, dtype=torch.float64, device=self._V.device)
            # precondition of functions.py:45 (the staged path does not run the fused check)
            mn, _ = vec_min_sum(x)
            assert mn >= 0, "DOptimalObj: x needs to be nonnegative"
            rc = self._lib.accbpg_dopt_eval_gram(self._h, _ptr(gram), int(flag), C.byref(fval), _ptr(g))
        _lib.check(rc, "accbpg_dopt_eval_gram")
        self.calls["value" if flag == 0 else "grad"] += 1
        if ent is not None:
            ent[3] = fval.value
        if flag == 0:
            return fval.value
        return g if flag == 1 else (fval.value, g)

    # ---- staged evaluation for design-point sharding ----
    def gram_into(self, x_dev, gram_dev):
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_gram(self._h, _ptr(x_dev), _ptr(gram_dev))
        _lib.check(rc, "accbpg_dopt_gram")

    def factor(self, gram_dev):
        fval = C.c_double(0.0)
        with torch.cuda.device(self._V.device):
            rc = self._lib.accbpg_dopt_factor(self._h, _ptr(gram_dev), C.byref(fval))
        _lib.check(rc, "accbpg_dopt_factor")
        return fval.value

    def grad_from_factor(self, g_dev):
        with torch.cuda.device(self._V.device):
            rc = self._lib.accbpg_dopt_grad(self._h, _ptr(g_dev))
        _lib.check(rc, "accbpg_dopt_grad")

    # ---- pieces used by D_opt_KYinit (accbpg/applications.py:79,84) ----
    def vt_times(self, q):
        """u = V^T q (np.dot(q, V)) for a length-m vector q -> length-n device vector."""
        qd, _ = to_dev(q)
        u = torch.empty(self.n, dtype=torch.float64, device=self._V.device)
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_vt_times(self._h, _ptr(qd), _ptr(u))
        _lib.check(rc, "accbpg_dopt_vt_times")
        return u

    def column(self, j):
        """V[:, j] as a NumPy vector."""
        out = torch.empty(self.m, dtype=torch.float64, device=self._V.device)
        with torch.cuda.device(self._V.device):
            rc = self._lib.accbpg_dopt_get_column(self._h, int(j), _ptr(out))
        _lib.check(rc, "accbpg_dopt_get_column")
        return out.cpu().numpy()

    def kyinit_picks(self, B, Q_out=None):
        """The 2m indices of the Kumar-Yildirim start for the m directions B[i] (accbpg_dopt_kyinit): all m steps on the
        device, one synchronisation.  ``Q_out``: optional m x m fp64 device tensor that receives the orthonormal
        directions, row j = Q[:, j]."""
        Bd, _ = to_dev(B)
        assert Bd.shape == (self.m, self.m), "kyinit_picks: B must be m x m"
        if Q_out is not None:
            assert Q_out.is_cuda and Q_out.dtype == torch.float64 and Q_out.is_contiguous() \
                and Q_out.shape == (self.m, self.m), "kyinit_picks: Q_out must be a contiguous m x m fp64 device tensor"
        picked = np.empty(2 * self.m, dtype=np.int64)
        with torch.cuda.device(self._V.device):
            self._lib.accbpg_dopt_set_stream(self._h, _stream())
            rc = self._lib.accbpg_dopt_kyinit(self._h, _ptr(Bd), picked.ctypes.data_as(C.POINTER(C.c_int64)),
                                              _ptr(Q_out))
        _lib.check(rc, "accbpg_dopt_kyinit")
        return picked

    # ---- kernel-time accounting used by bench.py ----
    def _handles(self):
        return [h for h in (self._h, getattr(self, "_h2", None)) if h]

    def profile(self, enable=True):
        """HIP-event timing of every kernel family on the stream it is launched on.  While it is on, the
        solvers keep F[k] = f(x) on their own stream (no side-stream overlap), so that the durations are those
        of kernels that have the chip to themselves."""
        self._prof = bool(enable)
        for h in self._handles():
            self._lib.accbpg_dopt_profile_enable(h, 1 if enable else 0)
            self._lib.accbpg_dopt_profile_reset(h)

    def profile_read(self):
        out = {}
        for idx, name in enumerate(["gram", "cholesky", "trtri", "grad", "gram_fixup", "fw_vpass"]):
            tot, num = 0.0, 0
            for h in self._handles():
                ms, cnt = C.c_double(0.0), C.c_int64(0)
                self._lib.accbpg_dopt_profile_read(h, idx, C.byref(ms), C.byref(cnt))
                tot, num = tot + ms.value, num + cnt.value
            out[name] = (tot, num)
        return out


class PoissonRegression(RSmoothFunction):
    """f(x) = D_KL(b, Ax) for the linear inverse problem A x = b  (accbpg/functions.py:85-120).

    ``A`` (m x n) and ``b`` may be NumPy arrays (copied to the GPU once) or fp64 CUDA tensors
    (borrowed); ``self.A``, ``self.b``, ``self.m``, ``self.n`` stay readable as in the reference.
    Each func_grad is two passes over A: A x with the KL terms fused into its epilogue, then A^T r."""

    _create, _destroy = "accbpg_poisson_create", "accbpg_poisson_destroy"
    _set_stream, _func_grad, _get_ax = "accbpg_poisson_set_stream", "accbpg_poisson_func_grad", "accbpg_poisson_get_ax"
    _size_msg = "PoissonRegression: x.size not equal to n."
    _match_msg = "A and b sizes not matching"

    def __init__(self, A, b):
        assert A.shape[0] == b.shape[0], self._match_msg
        self.A = A
        self.b = b
        self.m = A.shape[0]
        self.n = A.shape[1]
        self._A, _ = to_dev(A)
        self._b, _ = to_dev(b)
        lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self._A.device):
            rc = getattr(lib, self._create)(_ptr(self._A), self.m, self.n, self._A.stride(0), _ptr(self._b),
                                            _stream(), C.byref(h))
        _lib.check(rc, self._create)
        self._h = h
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                getattr(self._lib, self._destroy)(h)
            except Exception:
                pass
            self._h = None

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def func_grad(self, x, flag=2):
        size = x.numel() if isinstance(x, torch.Tensor) else x.size
        assert size == self.n, self._size_msg
        xd, was_np = to_dev(x)
        g = torch.empty(self.n, dtype=torch.float64, device=self._A.device) if flag != 0 else None
        fval = C.c_double(0.0)
        with torch.cuda.device(self._A.device):
            getattr(self._lib, self._set_stream)(self._h, _stream())
            rc = getattr(self._lib, self._func_grad)(self._h, _ptr(xd), int(flag), C.byref(fval), _ptr(g))
        _lib.check(rc, self._func_grad)
        if flag == 0:
            return fval.value
        if flag == 1:
            return from_dev(g, was_np)
        return fval.value, from_dev(g, was_np)

    def fitted(self):
        """A x of the last evaluation (length m) as a NumPy vector."""
        out = torch.empty(self.m, dtype=torch.float64, device=self._A.device)
        with torch.cuda.device(self._A.device):
            rc = getattr(self._lib, self._get_ax)(self._h, _ptr(out))
        _lib.check(rc, self._get_ax)
        return out.cpu().numpy()


class KLdivRegression(PoissonRegression):
    """f(x) = D_KL(Ax, b) for the nonnegative regression A x = b  (accbpg/functions.py:123-158).

    Same storage, device-tensor behaviour and two passes over A as PoissonRegression; only the per-row epilogue of
    the A x pass differs: r = log(Ax/b), t = Ax*log(Ax/b) - Ax + b, and g = A^T r."""
    _create, _destroy = "accbpg_kldiv_create", "accbpg_kldiv_destroy"
    _set_stream, _func_grad, _get_ax = "accbpg_kldiv_set_stream", "accbpg_kldiv_func_grad", "accbpg_kldiv_get_ax"
    _size_msg = "NonnegRegression: x.size not equal to n."
    _match_msg = "A and b size not matching"


class SVM_fun(RSmoothFunction):
    """f(x) = mean_i max(0, 1 - y_i (A x)_i) + (lamda/2) <x,x>, the soft-margin SVM (accbpg/functions.py:161-194).

    ``A`` (m x n) and ``y`` (length m, any numeric type) may be NumPy arrays (copied to the GPU once) or CUDA tensors
    (an fp64 ``A`` with unit column stride is borrowed with its row stride); ``self.lamda``, ``self.A`` and ``self.y``
    stay readable as in the reference, and ``lamda`` is read at every call.  Each func_grad is two passes over A: A x
    with the hinge terms in its epilogue, then A^T r with r_i = y_i where y_i (A x)_i < 1 (svm_kernels.hip).  The value
    is formed on the host as sum_t / m + lamda / 2 * <x,x>, the reference's operation order."""

    def __init__(self, lamda, A, y):
        self.lamda = lamda
        self.A = A
        self.y = y
        self.m = A.shape[0]
        self.n = A.shape[1]
        assert y.shape[0] == self.m, "SVM_fun: A and y sizes not matching"
        if isinstance(A, torch.Tensor) and A.is_cuda and A.dtype == torch.float64 and A.dim() == 2 \
                and (A.stride(1) == 1 or self.n == 1) and A.stride(0) >= self.n:
            self._A = A                                         # borrowed with its row stride
        else:
            self._A, _ = to_dev(A)
        self._y, _ = to_dev(y)
        self._y = self._y.to(self._A.device)
        lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self._A.device):
            rc = lib.accbpg_svm_create(_ptr(self._A), self.m, self.n, self._A.stride(0), _ptr(self._y), _stream(),
                                       C.byref(h))
        _lib.check(rc, "accbpg_svm_create")
        self._h = h
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.accbpg_svm_destroy(h)
            except Exception:
                pass
            self._h = None

    def _eval(self, x, flag, lamda):
        """The C entry at x: ((sum_t, <x,x>) or None, gradient tensor or None, x came from NumPy)."""
        size = x.numel() if isinstance(x, torch.Tensor) else x.size
        assert size == self.n, "SVM_fun: x.size not equal to n."
        xd, was_np = to_dev(x)
        xd = xd.reshape(-1)
        g = torch.empty(self.n, dtype=torch.float64, device=self._A.device) if flag != 0 else None
        fval = (C.c_double * 2)(0.0, 0.0)
        with torch.cuda.device(self._A.device):
            self._lib.accbpg_svm_set_stream(self._h, _stream())
            rc = self._lib.accbpg_svm_func_grad(self._h, _ptr(xd), float(lamda), int(flag), fval, _ptr(g))
        _lib.check(rc, "accbpg_svm_func_grad")
        sums = (np.float64(fval[0]), np.float64(fval[1])) if flag in (0, 2) else None
        return sums, g, was_np

    def _F_of(self, sums):
        return sums[0] / self.m + self.lamda / 2 * sums[1]      # np.mean(...) + lamda/2 * np.dot(x, x)

    def __call__(self, x):
        return self.F(x)

    def hinge_loss(self, x):
        sums, _, _ = self._eval(x, 0, 0.0)
        return sums[0] / self.m

    def F(self, x):
        sums, _, _ = self._eval(x, 0, 0.0)
        return self._F_of(sums)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def subgradient_loss(self, x):
        """mean_i 1[y_i (A x)_i < 1] y_i A_i (functions.py:179-181): the second pass without the lamda*x term."""
        _, g, was_np = self._eval(x, 3, 0.0)
        return from_dev(g, was_np)

    def func_grad(self, x, flag=2):
        """flag=0: function, flag=1: gradient, flag=2: function & gradient."""
        assert flag in (0, 1, 2), "SVM_fun: flag must be 0, 1 or 2."
        sums, g, was_np = self._eval(x, flag, self.lamda)
        if flag == 0:
            return self._F_of(sums)
        if flag == 1:
            return from_dev(g, was_np)
        return self._F_of(sums), from_dev(g, was_np)

    def margins(self):
        """A x of the last evaluation (length m) as a NumPy vector: y * margins() are the margins the hinge saw."""
        out = torch.empty(self.m, dtype=torch.float64, device=self._A.device)
        with torch.cuda.device(self._A.device):
            rc = self._lib.accbpg_svm_get_ax(self._h, _ptr(out))
        _lib.check(rc, "accbpg_svm_get_ax")
        return out.cpu().numpy()


class LogisticRegression(RSmoothFunction):
    """f(omega) = (1/m) sum_i log(1 + exp(-y_i (X omega)_i)), logistic regression (accbpg/functions.py:1068-1104,
    accbpg/ex_LR_L2L1Linf.py:19-54).

    ``X`` (m x n) and ``y`` (length m, any numeric type, usually +-1) may be NumPy arrays (copied to the GPU once) or
    CUDA tensors (an fp64 ``X`` with unit column stride is borrowed with its row stride); ``self.X``, ``self.y`` and
    ``self.alpha`` stay readable as in the reference.  Each func_grad is two passes over X: X omega with the logistic
    terms t_i = max(-s_i, 0) + log1p(exp(-|s_i|)) and r_i = -y_i sigma(-s_i), s_i = y_i (X omega)_i, in its epilogue,
    then X^T r / m (logistic_kernels.hip).  The value is formed on the host as sum_t / m."""

    def __init__(self, X, y, alpha=0.01):
        self.X = X
        self.y = y
        self.alpha = alpha
        self.m = X.shape[0]
        self.n = X.shape[1]
        assert y.shape[0] == self.m, "Logistic Regression: len(b) != m"
        if isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float64 and X.dim() == 2 \
                and (X.stride(1) == 1 or self.n == 1) and X.stride(0) >= self.n:
            self._A = X                                         # borrowed with its row stride
        else:
            self._A, _ = to_dev(X)
        self._y, _ = to_dev(y)
        self._y = self._y.to(self._A.device).reshape(-1)
        assert self._y.numel() == self.m, "Logistic Regression: len(b) != m"
        lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self._A.device):
            rc = lib.accbpg_logistic_create(_ptr(self._A), self.m, self.n, self._A.stride(0), _ptr(self._y), _stream(),
                                            C.byref(h))
        _lib.check(rc, "accbpg_logistic_create")
        self._h = h
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.accbpg_logistic_destroy(h)
            except Exception:
                pass
            self._h = None

    def _eval(self, omega, flag):
        """The C entry at omega: (sum_t or None, gradient tensor or None, omega came from NumPy)."""
        size = omega.numel() if isinstance(omega, torch.Tensor) else omega.size
        assert size == self.n, "Logistic Regression: x.size not equal to n"
        xd, was_np = to_dev(omega)
        xd = xd.reshape(-1)
        g = torch.empty(self.n, dtype=torch.float64, device=self._A.device) if flag != 0 else None
        fval = (C.c_double * 1)(0.0)
        with torch.cuda.device(self._A.device):
            self._lib.accbpg_logistic_set_stream(self._h, _stream())
            rc = self._lib.accbpg_logistic_func_grad(self._h, _ptr(xd), int(flag), fval, _ptr(g))
        _lib.check(rc, "accbpg_logistic_func_grad")
        return (np.float64(fval[0]) if flag != 1 else None), g, was_np

    def f(self, omega):
        return self.func_grad(omega, flag=0)

    def __call__(self, omega):
        return self.func_grad(omega, flag=0)

    def gradient(self, omega):
        return self.func_grad(omega, flag=1)

    def func_grad(self, omega, flag=2):
        """flag=0: function, flag=1: gradient, flag=2: function & gradient."""
        assert flag in (0, 1, 2), "Logistic Regression: flag must be 0, 1 or 2."
        sum_t, g, was_np = self._eval(omega, flag)
        if flag == 0:
            return sum_t / self.m
        if flag == 1:
            return from_dev(g, was_np)
        return sum_t / self.m, from_dev(g, was_np)

    # Margins along a segment.  After func_grad(x) the handle holds X x with its losses and weights; X (x + a d) is
    # X x + a (X d), so after one pass for X d every value on the segment, and the accepted point's rows, cost O(m).
    # A func_grad rebases the margins to its argument; the calls below raise ValueError on a handle that has none.
    def _line(self, name, *args):
        with torch.cuda.device(self._A.device):
            self._lib.accbpg_logistic_set_stream(self._h, _stream())
            rc = getattr(self._lib, name)(self._h, *args)
        _lib.check(rc, name)

    def line_begin(self, d):
        """Starts the segment x + a d from the point of the last func_grad (or line_accept): one pass for X d."""
        size = d.numel() if isinstance(d, torch.Tensor) else d.size
        assert size == self.n, "Logistic Regression: d.size not equal to n"
        dd, _ = to_dev(d)
        self._line("accbpg_logistic_line_begin", _ptr(dd.reshape(-1)))

    def line_value(self, a):
        """f(x + a d) from the carried margins fma(a, (X d)_i, (X x)_i); fitted(), losses() and weights() stay."""
        fval = (C.c_double * 1)(0.0)
        self._line("accbpg_logistic_line_value", float(a), fval)
        return np.float64(fval[0]) / self.m

    def line_accept(self, a):
        """Moves the handle's margins, losses and weights to x + a d; the next segment needs a new line_begin."""
        self._line("accbpg_logistic_line_accept", float(a))

    def func_grad_carried(self, flag=2, as_numpy=False):
        """func_grad at the point the handle's margins stand for, without the pass for X x: the value is the sum of
        the carried losses, the gradient X^T r / m.  The gradient is a CUDA tensor unless ``as_numpy``."""
        assert flag in (0, 1, 2), "Logistic Regression: flag must be 0, 1 or 2."
        g = torch.empty(self.n, dtype=torch.float64, device=self._A.device) if flag != 0 else None
        fval = (C.c_double * 1)(0.0)
        self._line("accbpg_logistic_func_grad_carried", int(flag), fval, _ptr(g))
        if flag == 0:
            return np.float64(fval[0]) / self.m
        if flag == 1:
            return from_dev(g, as_numpy)
        return np.float64(fval[0]) / self.m, from_dev(g, as_numpy)

    def _get(self, which):
        out = torch.empty(self.m, dtype=torch.float64, device=self._A.device)
        with torch.cuda.device(self._A.device):
            rc = self._lib.accbpg_logistic_get(self._h, which, _ptr(out))
        _lib.check(rc, "accbpg_logistic_get")
        return out.cpu().numpy()

    def fitted(self):
        """X omega of the last evaluation (length m) as a NumPy vector."""
        return self._get(0)

    def losses(self):
        """The per-row losses log(1 + exp(-y_i (X omega)_i)) of the last evaluation as a NumPy vector."""
        return self._get(1)

    def weights(self):
        """r_i = -y_i sigma(-y_i (X omega)_i) of the last evaluation as a NumPy vector: the gradient is X^T r / m."""
        return self._get(2)


class FrobeniusSymLoss(RSmoothFunction):
    """f(X) = 0.5*||M - X X^T||_F^2 for symmetric nonnegative matrix factorisation (accbpg/functions.py:908-976).

    ``M`` (n x n, symmetric) may be a NumPy array (copied to the GPU once) or an fp64 CUDA tensor (borrowed, any row
    stride >= n); ``X_init`` fixes the iterate shape n x r.  ``self.M``, ``self.M_norm`` and ``self.noise_level`` stay
    readable as in the reference.  Each evaluation is one fp64 MFMA pass over M for M X, with X^T X, X (X^T X), the
    gradient combine and the value's two sums in small launches behind it (symnmf_kernels.hip).  With a noise level,
    every call draws np.random.randn(*X.shape) from the legacy global generator, as the reference does (:961-964)."""

    def __init__(self, M, X_init, noise_level=None):
        if isinstance(M, torch.Tensor):
            assert bool(torch.allclose(M, M.T)), "Matrix M must be symmetric."
            self.M_norm = float(torch.linalg.norm(M.to(torch.float64)))
        else:
            assert np.allclose(M, M.T), "Matrix M must be symmetric."
            self.M_norm = np.linalg.norm(M)
        self.M = M
        self.noise_level = noise_level
        self.n = M.shape[0]
        self.shape = tuple(X_init.shape)
        assert len(self.shape) == 2 and self.shape[0] == self.n, "FrobeniusSymLoss: X_init must be n x r."
        self.r = self.shape[1]
        if isinstance(M, torch.Tensor) and M.is_cuda and M.dtype == torch.float64 and M.stride(1) == 1 \
                and M.stride(0) >= self.n:
            self._M = M                                         # borrowed with its row stride
        else:
            self._M, _ = to_dev(M)
        lib = _lib.load()
        h = C.c_void_p()
        with torch.cuda.device(self._M.device):
            rc = lib.accbpg_symnmf_create(_ptr(self._M), self.n, self._M.stride(0), self.r, float(self.M_norm),
                                          _stream(), C.byref(h))
        _lib.check(rc, "accbpg_symnmf_create")
        self._h = h
        self._lib = lib

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                self._lib.accbpg_symnmf_destroy(h)
            except Exception:
                pass
            self._h = None

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def plan(self):
        """(k pieces of the M X product, rows per piece, wide tile, row chunks of X^T X) of this handle."""
        out = (C.c_int64 * 4)()
        _lib.check(self._lib.accbpg_symnmf_plan(self._h, out), "accbpg_symnmf_plan")
        return tuple(out)

    def func_grad(self, X, flag=2):
        """flag=0: function, flag=1: gradient, flag=2: function & gradient."""
        noise = None
        if self.noise_level is not None:
            noise = (np.random.randn(*X.shape) - 0.5) * self.noise_level        # functions.py:964
        assert tuple(X.shape) == self.shape, "FrobeniusSymLoss: X.shape not equal to (n, r)."
        xd, was_np = to_dev(X)
        fval = C.c_double(0.0)
        g = torch.empty(self.shape, dtype=torch.float64, device=self._M.device) if flag != 0 else None
        with torch.cuda.device(self._M.device):
            self._lib.accbpg_symnmf_set_stream(self._h, _stream())
            rc = self._lib.accbpg_symnmf_func_grad(self._h, _ptr(xd), int(flag), C.byref(fval), _ptr(g))
        _lib.check(rc, "accbpg_symnmf_func_grad")
        if flag == 0:
            return np.float64(fval.value)
        if noise is not None:
            nd, _ = to_dev(noise)
            g = vec_axpby(1.0, g, 1.0, nd)                                    # g + noise_vector
        g = from_dev(g, was_np)
        return g if flag == 1 else (np.float64(fval.value), g)


# ------------------------------------------------------------------ h
class LegendreFunction:
    """Legendre kernel protocol (accbpg/functions.py:199-235)."""

    def __call__(self, x):
        assert 0, "LegendreFunction: __call__(x) is not defined."

    def extra_Psi(self, x):
        return 0

    def gradient(self, x):
        assert 0, "LegendreFunction: gradient(x) is not defined."

    def divergence(self, x, y):
        assert 0, "LegendreFunction: divergence(x,y) is not defined."

    def prox_map(self, g, L):
        assert 0, "LegendreFunction: prox_map(x, L) is not defined."

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g should have same size."
        assert L > 0, "Relative smoothness constant L should be positive."
        return self.prox_map(g - L * self.gradient(y), L)


class BurgEntropy(LegendreFunction):
    """h(x) = -sum log x_i  (accbpg/functions.py:238-271)."""

    def __call__(self, x):
        # off the solver path (no solver calls h(x)); evaluated with torch on the device
        xd, _ = to_dev(x)
        assert float(xd.min()) > 0, "BurgEntropy only takes positive arguments."
        return float(-torch.log(xd).sum())

    def gradient(self, x):
        xd, was_np = to_dev(x)
        assert float(xd.min()) > 0, "BurgEntropy only takes positive arguments."
        return from_dev(-1.0 / xd, was_np)

    def divergence(self, x, y):
        assert x.shape == y.shape, "Vectors x and y are of different sizes."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        n = xd.numel()
        out = C.c_double(0.0)
        _call("accbpg_burg_divergence", xd, _ptr(xd), _ptr(yd), n, C.byref(out), _WS,
              assert_msg="Entries of x or y not positive.")
        return np.float64(out.value)                            # a NumPy scalar, as the reference's sum is (:253)

    _kind = 0       # closed-form variant of accbpg_burg_reg_div_prox
    lamda = 0

    def _reg_prox(self, y, g, L):
        gd, was_np = to_dev(g)
        yd = None
        if y is not None:
            yd, _ = to_dev(y)
        out = torch.empty_like(gd)
        with torch.cuda.device(gd.device):
            rc = _lib.load().accbpg_burg_reg_div_prox(self._kind, _ptr(yd), _ptr(gd), float(L), float(self.lamda),
                                                      gd.numel(), _ptr(out), _stream())
        _lib.check(rc, "accbpg_burg_reg_div_prox")
        return from_dev(out, was_np)

    def prox_map(self, g, L):
        assert L > 0, "BurgEntropy prox_map only takes positive L value."
        return self._reg_prox(None, g, L)       # g.min() > 0 is checked on the device (functions.py:261)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different sizes."
        assert L > 0, "Either y or L is not positive."
        return self._reg_prox(y, g, L)          # y.min() > 0 is checked on the device (functions.py:270)


class BurgEntropyL1(BurgEntropy):
    """Burg entropy for min_{x>0} f(x) + lamda*||x||_1  (accbpg/functions.py:274-298)."""
    _kind = 1

    def __init__(self, lamda=0, x_max=1e4):
        assert lamda >= 0, "BurgEntropyL1: lambda should be nonnegative."
        self.lamda = lamda
        self.x_max = x_max

    def extra_Psi(self, x):
        if self.lamda == 0:
            return 0.0
        xd, _ = to_dev(x)
        return self.lamda * vec_min_sum(xd)[1]

    def prox_map(self, g, L):
        assert L > 0, "BurgEntropyL1: prox_map only takes positive L."
        return self._reg_prox(None, g, L)       # g.min() > -lamda is checked on the device (:296)


class BurgEntropyL2(BurgEntropy):
    """Burg entropy for min_{x>0} f(x) + (lamda/2)*||x||_2^2  (accbpg/functions.py:301-323)."""
    _kind = 2

    def __init__(self, lamda=0):
        assert lamda >= 0, "BurgEntropyL2: lamda should be nonnegative."
        self.lamda = lamda

    def extra_Psi(self, x):
        if self.lamda == 0:
            return 0.0
        xd, _ = to_dev(x)
        return (self.lamda / 2) * vec_dot(xd, xd)

    def prox_map(self, g, L):
        assert L > 0, "BurgEntropyL2: prox_map only takes positive L value."
        return self._reg_prox(None, g, L)


class BurgEntropySimplex(BurgEntropy):
    r"""Burg entropy with the unit-simplex constraint (accbpg/functions.py:326-356)."""

    def __init__(self, eps=1e-8):
        assert eps > 0, "BurgEntropySimplex: eps should be positive."
        self.eps = eps
        self.last_info = (0, 0)     # (bisection steps, Newton steps) of the last prox

    def _prox(self, y, g, L):
        gd, was_np = to_dev(g)
        yd = None
        if y is not None:
            yd, _ = to_dev(y)
        n = gd.numel()
        out = torch.empty(n, dtype=torch.float64, device=gd.device)
        info = (C.c_int * 2)(0, 0)
        _call("accbpg_burg_simplex_div_prox", gd, _ptr(yd), _ptr(gd), float(L), float(self.eps), n, _ptr(out), _WS,
              info, assert_msg="Either y or L is not positive.")
        self.last_info = (info[0], info[1])
        return from_dev(out, was_np)

    def prox_map(self, g, L):
        assert L > 0, "BergEntropySimplex prox_map only takes positive L."
        return self._prox(None, g, L)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different sizes."
        assert L > 0, "Either y or L is not positive."
        return self._prox(y, g, L)


    def prox_map_acc(self, xi, alpha, g):
        """(xi + alpha*g, prox_map(xi + alpha*g, 1)) in one call on device vectors: AIBM's
        ``xi_grad += alpha*grad_x; z_k = h.prox_map(xi_grad, 1)`` (accbpg/algorithms.py:630-631).  The prox is the one
        of ``prox_map``, bit for bit; nothing is read back."""
        n = xi.numel()
        xi_out = torch.empty_like(xi)
        out = torch.empty_like(xi)
        _call("accbpg_burg_simplex_prox_acc", xi, _ptr(xi), float(alpha), _ptr(g), 1.0, float(self.eps), n,
              _ptr(xi_out), _ptr(out), _WS, None)
        return xi_out, out


class ShannonEntropy(LegendreFunction):
    """h(x) = sum x_i log x_i for x >= 0, h(0) = 0  (accbpg/functions.py:398-438).  ``delta`` guards the
    logarithms of the divergence at exact zeros."""
    _kind = 0       # variant of accbpg_shannon_div_prox
    lamda = 0

    def __init__(self, delta=1e-20):
        self.delta = delta

    def __call__(self, x):
        # off the solver path (no solver calls h(x)); evaluated with torch on the device
        xd, _ = to_dev(x)
        assert float(xd.min()) >= 0, "ShannonEntropy takes nonnegative arguments."
        xx = torch.clamp(xd, min=self.delta)
        return float((xx * torch.log(xx)).sum())

    def gradient(self, x):
        xd, was_np = to_dev(x)
        assert float(xd.min()) >= 0, "ShannonEntropy takes nonnegative arguments."
        return from_dev(1.0 + torch.log(torch.clamp(xd, min=self.delta)), was_np)

    def divergence(self, x, y):
        assert x.shape == y.shape, "Vectors x and y are of different shapes."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        n = xd.numel()
        out = C.c_double(0.0)
        _call("accbpg_shannon_divergence", xd, _ptr(xd), _ptr(yd), n, float(self.delta), C.byref(out), _WS,
              assert_msg="Some entries are negative.")
        return np.float64(out.value)                            # a NumPy scalar, as the reference's sum is (:421)

    def _prox(self, y, g, L, msg):
        gd, was_np = to_dev(g)
        yd = None
        if y is not None:
            yd, _ = to_dev(y)
        n = gd.numel()
        out = torch.empty_like(gd)
        _call("accbpg_shannon_div_prox", gd, self._kind, _ptr(yd), _ptr(gd), float(L), float(self.lamda), n, _ptr(out),
              _WS if self._kind == 2 else _ptr(None), assert_msg=msg)
        return from_dev(out, was_np)

    def prox_map(self, g, L):
        assert L > 0, "ShannonEntropy prox_map require L > 0."
        return self._prox(None, g, L, None)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different sizes."
        assert L > 0, "Some entries of y are negavie."
        return self._prox(y, g, L, "Some entries of y are negavie.")    # y.min() >= 0 on the device (:437)


class ShannonEntropyL1(ShannonEntropy):
    """Shannon entropy for min_{x >= 0} f(x) + lamda*||x||_1  (accbpg/functions.py:441-466): the prox maps
    take lamda + g."""
    _kind = 1

    def __init__(self, lamda=0, delta=1e-20):
        ShannonEntropy.__init__(self, delta)
        self.lamda = lamda

    def extra_Psi(self, x):
        if self.lamda == 0:
            return 0.0
        xd, _ = to_dev(x)
        return self.lamda * vec_min_sum(xd)[1]


class ShannonEntropySimplex(ShannonEntropy):
    """Shannon entropy with the unit-simplex constraint (accbpg/functions.py:469-490): the prox maps of
    ShannonEntropy divided by their sum."""
    _kind = 2

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different shapes."
        assert L > 0, "prox_map needs positive arguments."
        return self._prox(y, g, L, "prox_map needs positive arguments.")   # y.min() > 0 on the device (:488)


class SumOf2nd4thPowers(LegendreFunction):
    """h(x) = (sigma/2)||x||^2 + (alpha/4)||x||^4 on vectors or n x r matrices (Frobenius norm), accbpg/functions.py:
    493-555.  The norms come from device sums of squares; the scalar recurrences (norm**4, norm**2, the cubic of the
    prox map) run on the host in float64 with the reference's formulas."""
    _clip = 0
    upper_bound = None

    def __init__(self, alpha, sigma):
        self.alpha = alpha
        self.sigma = sigma

    def _norm(self, xd):
        return np.sqrt(np.float64(vec_dot(xd, xd)))

    def _h_of_norm(self, norm):
        return (self.alpha / 4) * norm ** 4 + self.sigma / 2 * norm ** 2

    def __call__(self, x):
        xd, _ = to_dev(x)
        return self._h_of_norm(self._norm(xd))

    def gradient(self, x):
        xd, was_np = to_dev(x)
        norm = self._norm(xd)
        return from_dev(vec_axpby(self.sigma + self.alpha * norm ** 2, xd, 0.0, xd), was_np)

    def _divergence_of(self, nx2, ny2, ydiff):
        """h(x) - (h(y) + <grad h(y), x - y>) from ||x||^2, ||y||^2 and <y, x - y> (functions.py:518-521)."""
        ny = np.sqrt(np.float64(ny2))
        c = self.sigma + self.alpha * ny ** 2
        return self._h_of_norm(np.sqrt(np.float64(nx2))) - (self._h_of_norm(ny) + c * ydiff)

    def divergence(self, x, y):
        assert x.shape == y.shape, "Bregman div: x and y not same shape."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        o = quartic_ls_terms(None, xd, yd)
        return self._divergence_of(o[1], o[2], o[3])

    def ls_terms(self, g, x, y, z=None, z1=None):
        """(<g,x-y>, D(x,y), D(z,z1)) in one launch and one readback."""
        o = quartic_ls_terms(g, x, y, z, z1)
        dzz = self._divergence_of(o[4], o[5], o[6]) if z is not None else 0.0
        return np.float64(o[0]), self._divergence_of(o[1], o[2], o[3]), dzz

    def solve_cubic(self, c, alpha):
        """The real root of z^3 - alpha*z^2 = c, c > 0 (functions.py:522-544), on the host."""
        z = alpha / 3.0
        alpha3 = alpha ** 3
        delta = c ** 2 + 4 * alpha3 * c / 27.0
        sq_delta = np.sqrt(delta)
        b = 0.5 * c + alpha3 / 27.0
        z += np.cbrt(b + 0.5 * sq_delta)
        z += np.cbrt(b - 0.5 * sq_delta)
        return z

    def div_prox_map(self, y, g, L):
        yd, was_np = to_dev(y)
        gd, _ = to_dev(g)
        z = self.alpha * self._norm(yd) ** 2 + self.sigma                     # :551
        n = yd.numel()
        out = torch.empty_like(yd)
        ssq = C.c_double(0.0)
        ub = np.inf if self.upper_bound is None else float(self.upper_bound)
        _call("accbpg_quartic_prox_stage", yd, _ptr(yd), _ptr(gd), float(z), float(1 / L), self._clip, ub, n, _ptr(out),
              C.byref(ssq), _WS)
        norm = np.sqrt(np.float64(ssq.value))
        z = self.solve_cubic(self.alpha * norm ** 2, self.sigma)                 # :554
        return from_dev(vec_div_scalar(out, z), was_np)


class SumOf2nd4thPowersPositiveOrthant(SumOf2nd4thPowers):
    """SumOf2nd4thPowers on the nonnegative orthant (accbpg/functions.py:558-577): the prox map clips
    z*y - g/L to [0, upper_bound] before the cubic."""
    _clip = 1

    def __init__(self, alpha, sigma, upper_bound=None):
        self.alpha = alpha
        self.sigma = sigma
        self.upper_bound = upper_bound


class SquaredL2Norm(LegendreFunction):
    """h(x) = (1/2)||x||_2^2 (accbpg/functions.py:738-759), composed from the vector kernels."""

    def __call__(self, x):
        xd, _ = to_dev(x)
        return 0.5 * vec_dot(xd, xd)

    def gradient(self, x):
        return x

    def divergence(self, x, y):
        assert x.shape == y.shape, "SquaredL2Norm: x and y not same shape."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        xy = vec_axpby(1.0, xd, -1.0, yd)
        return 0.5 * vec_dot(xy, xy)

    def prox_map(self, g, L):
        assert L > 0, "SquaredL2Norm: L should be positive."
        gd, was_np = to_dev(g)
        return from_dev(vec_axpby(-(1 / L), gd, 0.0, gd), was_np)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape and L > 0, "Vectors y and g not same shape."
        yd, was_np = to_dev(y)
        gd, _ = to_dev(g)
        return from_dev(vec_axpby(1.0, yd, -(1 / L), gd), was_np)


class L2L1Linf(LegendreFunction):
    """h(x) = (1/2)||x||_2^2 for problems  minimize f(x) + lamda*||x||_1  subject to ||x||_inf <= B
    (accbpg/functions.py:782-835).  ``lamda`` and ``B`` are read at every call.  The prox maps are one elementwise
    launch in the reference's operation order (soft threshold at lamda/L, then the clip to [-B, B]); the sums run on
    the fixed tree of the vector kernels."""

    def __init__(self, lamda=0, B=1):
        self.lamda = lamda
        self.B = B

    def __call__(self, x):
        xd, _ = to_dev(x)
        return 0.5 * vec_dot(xd, xd)

    def extra_Psi(self, x):
        """lamda * ||x||_1"""
        xd, _ = to_dev(x)
        return self.lamda * l1_norm(xd)

    def gradient(self, x):
        return x

    def divergence(self, x, y):
        """D(x, y) = (1/2)||x - y||_2^2"""
        assert x.shape == y.shape, "L2L1Linf: x and y not same shape."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        return sq_ls_terms(None, xd, yd)[1]

    def ls_terms(self, g, x, y, z=None, z1=None):
        """(<g,x-y>, D(x,y), D(z,z1)) in one launch and one readback."""
        return sq_ls_terms(g, x, y, z, z1)

    def _prox(self, y, g, L):
        gd, was_np = to_dev(g)
        yd = to_dev(y)[0] if y is not None else None
        out = torch.empty_like(gd)
        _call("accbpg_l2l1linf_prox", gd, _ptr(yd), _ptr(gd), float(L), float(self.lamda), float(self.B), gd.numel(),
              _ptr(out), assert_msg="L2L1Linf: L should be positive.")
        return from_dev(out, was_np)

    def prox_map(self, g, L):
        """argmin_{||x||_inf <= B} { lamda*||x||_1 + <g, x> + L*h(x) }"""
        assert L > 0, "L2L1Linf: L should be positive."
        return self._prox(None, g, L)

    def div_prox_map(self, y, g, L):
        """argmin_{||x||_inf <= B} { lamda*||x||_1 + <g, x> + L*D(x, y) }"""
        assert y.shape == g.shape and L > 0, "Vectors y and g not same shape."
        return self._prox(y, g, L)


def polydiv_prox_radius(L, lamda, ds_mean, ds_mean_quad, radius):
    """t* = min(radius, t^) with t^ >= 0 the root of L*phi'(t) = radius, phi'(t) = lamda^2 t^3 + 2 lamda ds_mean t^2 +
    ds_mean_quad t: the norm of the minimiser of L*phi(||x||) + <g', x> over ||x|| <= radius when ||g'|| = radius
    (PolyDiv.prox_map).  phi' is increasing and convex on t >= 0, so Newton from the right end of [0, radius] descends
    monotonically to the root; an iterate that leaves the bracket is replaced by its midpoint."""
    a3, a2, a1 = float(lamda) ** 2, 2.0 * float(lamda) * float(ds_mean), float(ds_mean_quad)
    L, radius = float(L), float(radius)

    def resid(t):
        return L * (((a3 * t + a2) * t + a1) * t) - radius

    if not resid(radius) > 0.0:                     # t^ >= radius (or a NaN coefficient): the ball's boundary
        return radius
    lo, hi, t = 0.0, radius, radius                 # resid(lo) < 0 < resid(hi)
    for _ in range(200):
        r = resid(t)
        if r > 0.0:
            hi = t
        elif r < 0.0:
            lo = t
        else:
            return t
        slope = L * ((3.0 * a3 * t + 2.0 * a2) * t + a1)
        nxt = t - r / slope if slope > 0.0 else 0.5 * (lo + hi)
        if not lo < nxt < hi:
            nxt = 0.5 * (lo + hi)
        if nxt == t or hi - lo <= 0.0:
            return t
        if abs(nxt - t) <= 1e-17 * abs(t):
            return nxt
        t = nxt
    return t


class PolyDiv(LegendreFunction):
    """h(x) = lamda^2/4 ||x||^4 + 2 lamda DS_mean/3 ||x||^3 + DS_mean_quad/2 ||x||^2 on the ball ||x|| <= radius
    (accbpg/functions.py:838-905; arXiv 1710.04718 (27)), DS_mean and DS_mean_quad the mean row norm of the dataset and
    the mean of its square, computed on the host once.

    The norms come from device sums; the scalar formulas run on the host in float64 as the reference writes them.
    ``gradient`` keeps the reference's factor lamda**4*||x||**2 + 2*lamda*DS_mean + DS_mean_quad, which is not the
    derivative of h, and ``divergence`` is built on it, as in the reference.  ``prox_map`` returns the exact minimiser
    of the problem the reference hands to a conic solver: with g' = g/||g||*radius it is x = -t* g/||g||,
    t* = polydiv_prox_radius(...)."""

    def __init__(self, DS, lamda=0, radius=1):
        self.lamda = lamda
        self.radius = radius
        self.DS = DS
        ds = DS.detach().cpu().numpy() if isinstance(DS, torch.Tensor) else DS
        self.DS_mean = np.mean(np.linalg.norm(ds, axis=1))
        self.DS_mean_quad = np.mean(np.linalg.norm(ds, axis=1) ** 2)

    def _h_of_norm(self, norm):
        norm4 = 1 / 4 * norm ** 4
        norm3 = 1 / 3 * norm ** 3
        norm2 = 1 / 2 * norm ** 2
        return self.lamda ** 2 * norm4 + 2 * self.lamda * self.DS_mean * norm3 + self.DS_mean_quad * norm2

    def _grad_factor(self, sq):
        """the scalar in front of x in gradient(x), from ||x||^2"""
        return self.lamda ** 4 * np.sqrt(np.float64(sq)) ** 2 + 2 * self.lamda * self.DS_mean + self.DS_mean_quad

    def __call__(self, x):
        return self.h(x)

    def h(self, x):
        xd, _ = to_dev(x)
        return self._h_of_norm(np.sqrt(np.float64(vec_dot(xd, xd))))

    def extra_Psi(self, x):
        return 0

    def gradient(self, x):
        xd, was_np = to_dev(x)
        return from_dev(vec_axpby(self._grad_factor(vec_dot(xd, xd)), xd, 0.0, xd), was_np)

    def _divergence_of(self, nx2, ny2, ydiff):
        """h(x) - h(y) - <gradient(y), x - y> from ||x||^2, ||y||^2 and <y, x - y>"""
        return self._h_of_norm(np.sqrt(np.float64(nx2))) - self._h_of_norm(np.sqrt(np.float64(ny2))) \
            - self._grad_factor(ny2) * ydiff

    def divergence(self, x, y):
        assert x.shape == y.shape, "PolyDivBall: x and y not same shape."
        xd, _ = to_dev(x)
        yd, _ = to_dev(y)
        o = quartic_ls_terms(None, xd, yd)
        return self._divergence_of(o[1], o[2], o[3])

    def ls_terms(self, g, x, y, z=None, z1=None):
        """(<g,x-y>, D(x,y), D(z,z1)) in one launch and one readback."""
        o = quartic_ls_terms(g, x, y, z, z1)
        dzz = self._divergence_of(o[4], o[5], o[6]) if z is not None else 0.0
        return np.float64(o[0]), self._divergence_of(o[1], o[2], o[3]), dzz

    def _prox_radius(self, L):
        return polydiv_prox_radius(L, self.lamda, self.DS_mean, self.DS_mean_quad, self.radius)

    def prox_map(self, g, L):
        gd, was_np = to_dev(g)
        g_norm = np.sqrt(np.float64(vec_dot(gd, gd)))
        if g_norm == 0.0:
            g_norm = 1e-8                                                      # functions.py:873-874
        return from_dev(vec_axpby(-(self._prox_radius(L) / g_norm), gd, 0.0, gd), was_np)

    def div_prox_map(self, y, g, L):
        """prox_map(g - L*gradient(y), L): out = c_y*y - g/L = -(g - L*c_y*y)/L and its norm from one launch, then
        x = t* out/||out||."""
        yd, was_np = to_dev(y)
        gd, _ = to_dev(g)
        c = self._grad_factor(vec_dot(yd, yd))
        out = torch.empty_like(yd)
        ssq = C.c_double(0.0)
        _call("accbpg_quartic_prox_stage", yd, _ptr(yd), _ptr(gd), float(c), float(1 / L), 0, np.inf, yd.numel(),
              _ptr(out), C.byref(ssq), _WS)
        norm = np.sqrt(np.float64(ssq.value))
        if norm == 0.0:
            norm = 1e-8
        return from_dev(vec_axpby(self._prox_radius(L) / norm, out, 0.0, out), was_np)


# ------------------------------------------------------------------ vector helpers for the solver loops
def vec_axpby(a, x, b, z):
    """a*x + b*z with NumPy's rounding (two products, one sum)."""
    out = torch.empty_like(x)
    _call("accbpg_vec_axpby", x, float(a), _ptr(x), float(b), _ptr(z), x.numel(), _ptr(out))
    return out


def vec_dot_diff(g, x, y):
    """<g, x - y>  (np.dot(g, x1-x), algorithms.py:53)."""
    out = C.c_double(0.0)
    _call("accbpg_vec_dot_diff", x, _ptr(g), _ptr(x), _ptr(y), x.numel(), C.byref(out), _WS)
    return out.value


def vec_dot(x, y):
    """<x, y>  (np.dot(x, x) of BurgEntropyL2.extra_Psi, functions.py:314)."""
    out = C.c_double(0.0)
    _call("accbpg_vec_dot", x, _ptr(x), _ptr(y), x.numel(), C.byref(out), _WS)
    return out.value


def ls_terms(g, x, y, z=None, z1=None):
    """(<g,x-y>, D(x,y), D(z,z1)) in one launch and one readback."""
    out = (C.c_double * 3)(0.0, 0.0, 0.0)
    _call("accbpg_ls_terms", x, _ptr(g), _ptr(x), _ptr(y), _ptr(z), _ptr(z1), x.numel(), out, _WS,
          assert_msg="Entries of x or y not positive.")
    # NumPy scalars, as the reference's sums are (accbpg/functions.py:253): D(x+,y) / D(z+,z) with D(z+,z) == 0 --
    # an iterate that has stopped moving -- is then inf or nan with a warning, as in the reference, not an exception
    # (the stopping rule dzz < epsilon right behind it ends the run, accbpg/algorithms.py:155,174)
    return np.float64(out[0]), np.float64(out[1]), np.float64(out[2])


def combine_ls_terms(h, a, u, b, v, c, g=None, x=None):
    """w = (a*u + b*v)/c with NumPy's rounding, and (<g, w - x>, D_h(w, x)) from the same pass and one read-back when x
    is given; h is this package's Burg entropy (any variant) or SquaredL2Norm.  Returns (w, lin, dist); lin and dist
    are None without x."""
    kind = 1 if isinstance(h, SquaredL2Norm) else 0
    w = torch.empty_like(u)
    out = (C.c_double * 2)(0.0, 0.0)
    _call("accbpg_combine_ls_terms", u, kind, float(a), _ptr(u), float(b), _ptr(v), float(c), _ptr(g), _ptr(x),
          u.numel(), _ptr(w), out, _WS if x is not None else _ptr(None), assert_msg="Entries of x or y not positive.")
    if x is None:
        return w, None, None
    return w, np.float64(out[0]), np.float64(out[1])


def shannon_ls_terms(g, x, y, z=None, z1=None, delta=1e-20):
    """(<g,x-y>, D(x,y), D(z,z1)) of the Shannon entropy in one streaming pass and one readback (g None: 0)."""
    out = (C.c_double * 3)(0.0, 0.0, 0.0)
    _call("accbpg_shannon_ls_terms", x, _ptr(g), _ptr(x), _ptr(y), _ptr(z), _ptr(z1), x.numel(), float(delta), out,
          _WS, assert_msg="Some entries are negative.")
    return np.float64(out[0]), np.float64(out[1]), np.float64(out[2])


def quartic_ls_terms(g, x, y, z=None, z1=None):
    """(<g,x-y>, ||x||^2, ||y||^2, <y,x-y>, ||z||^2, ||z1||^2, <z1,z-z1>) in one streaming pass and one readback."""
    out = (C.c_double * 7)()
    _call("accbpg_quartic_ls_terms", x, _ptr(g), _ptr(x), _ptr(y), _ptr(z), _ptr(z1), x.numel(), out, _WS)
    return tuple(out)


def l1_norm(x):
    """sum |x_i|  (np.sum(abs(x)) of L2L1Linf.extra_Psi, functions.py:801)."""
    out = C.c_double(0.0)
    _call("accbpg_l1_norm", x, _ptr(x), x.numel(), C.byref(out), _WS)
    return np.float64(out.value)


def sq_ls_terms(g, x, y, z=None, z1=None):
    """(<g,x-y>, (1/2)||x-y||^2, (1/2)||z-z1||^2) in one streaming pass and one readback (g None, z None: 0)."""
    xd, yd = to_dev(x)[0], to_dev(y)[0]
    gd = to_dev(g)[0] if g is not None else None
    zd = to_dev(z)[0] if z is not None else None
    z1d = to_dev(z1)[0] if z is not None else None
    out = (C.c_double * 3)(0.0, 0.0, 0.0)
    _call("accbpg_sq_ls_terms", xd, _ptr(gd), _ptr(xd), _ptr(yd), _ptr(zd), _ptr(z1d), xd.numel(), out, _WS)
    return np.float64(out[0]), np.float64(out[1]), np.float64(out[2])


def vec_min_sum(x):
    out = (C.c_double * 2)(0.0, 0.0)
    _call("accbpg_vec_min_sum", x, _ptr(x), x.numel(), out, _WS)
    return out[0], out[1]


def vec_div_scalar(x, d):
    """x / d elementwise (NumPy true division)."""
    out = torch.empty_like(x)
    _call("accbpg_vec_div_scalar", x, _ptr(x), float(d), x.numel(), _ptr(out))
    return out


def vec_argminmax(x):
    """(first argmin, first argmax, min, max) of a device vector."""
    idx = (C.c_int64 * 2)(0, 0)
    val = (C.c_double * 2)(0.0, 0.0)
    _call("accbpg_vec_argminmax", x, _ptr(x), x.numel(), idx, val, _WS)
    return idx[0], idx[1], val[0], val[1]


def vec_vertex(idx, value, fill, n, device):
    out = torch.empty(n, dtype=torch.float64, device=device)
    _call("accbpg_vec_vertex", out, int(idx), float(value), float(fill), int(n), _ptr(out))
    return out
