"""Outer loops of BPG / ABPG / ABPG_gain / ABPG_expo / ABDA and of the inexact-oracle accelerated
methods AIBM / AdaptFGM / UniversalGM with the reference's signatures, defaults, return tuples,
print tables and quirks (accbpg/algorithms.py:11-514, 593-777), running on device vectors.  The host keeps the iteration and every scalar decision; all
length-n and matrix work goes through libaccbpg_hip.so via the f / h objects of
``functions.py`` and the fused vector helpers there.

``x0`` may be a NumPy array (results come back as NumPy) or an fp64 CUDA tensor
(results stay on the device).  ``T[k]`` is the time at which ``F[k]`` was known on the
host, as the reference stamps it right after computing ``F[k]``: read off the host clock
when f(x) runs on the solver's stream, and corrected by the device-reported lead when it
ran on the side stream beside the gradient evaluation (``DOptimalObj.overlap_values``,
the default) -- see ``_stamp``.
"""
from __future__ import annotations

import math
import time

import numpy as np
import torch

from .functions import (BurgEntropy, BurgEntropySimplex, DOptimalObj, L2L1Linf, PolyDiv, ShannonEntropy, SquaredL2Norm,
                        SumOf2nd4thPowers,
                        combine_ls_terms, from_dev, ls_terms, shannon_ls_terms, to_dev, vec_axpby, vec_div_scalar,
                        vec_dot_diff)
from .solver_runs import (ACCEPT, BREAK, NEEDS_VALUE, _ABDARun, _ABPGRun, _BPGRun, _ExpoRun, _GainRun,  # noqa: F401
                          next_theta, solve_theta)
from .utils import get_random_float


def _divergences(h, g, x, y, z, z_prev):
    """(<g, x-y>, D(x,y), D(z,z_prev)); one fused launch when h is this package's Burg, Shannon or quartic kernel
    (g None: no inner product, z None: no second divergence).  Inner products of n x r iterates are flat."""
    if isinstance(h, BurgEntropy):
        return ls_terms(g, x, y, z, z_prev)
    if isinstance(h, ShannonEntropy):
        return shannon_ls_terms(g, x, y, z, z_prev, h.delta)
    if isinstance(h, (SumOf2nd4thPowers, PolyDiv, L2L1Linf)):
        return h.ls_terms(g, x, y, z, z_prev)
    lin = vec_dot_diff(g, x, y) if g is not None else 0.0
    return lin, h.divergence(x, y), (h.divergence(z, z_prev) if z is not None else 0.0)


def _lin(f):
    """True when f is this package's D-optimal objective with Gram-matrix reuse switched on."""
    return bool(getattr(f, "_lin", False))


def _value(f, x, combo=None):
    return f.func_grad_combo(x, combo, 0) if _lin(f) else f(x)


def _value_begin(f, x, combo):
    """F[k] = f(x) does not feed the gradient evaluation at y: it is started on the objective's side stream
    (DOptimalObj.overlap_values, the default) unless that is switched off or kernel timing is on
    (DOptimalObj.profile), in which case it is evaluated now."""
    if (not _lin(f)) and getattr(f, "_overlap", False) and not getattr(f, "_prof", False) \
            and isinstance(x, torch.Tensor) and x.is_cuda:
        if getattr(f, "_memo_on", False):                       # opt-in: f at this very tensor was the last value computed
            hit = f._memo_get(x)
            if hit is not None:
                return ("value", hit)
        return ("ticket", f.value_async(x))
    return ("value", _value(f, x, combo))


def _can_speculate(f, x, checkdiv):
    """Gradient evaluations may be started ahead of the line-search decision on this package's D-optimal objective
    when the caller has switched that on (DOptimalObj.speculate -- opt-in: measured slower at (2048,32768), 47.7
    against 50.5 it/s, and 3 % faster at (512,8192)) and it evaluates directly, on the device, with the side stream
    in use."""
    return (not checkdiv) and (not _lin(f)) and getattr(f, "_spec", False) and getattr(f, "_overlap", False) \
        and not getattr(f, "_prof", False) and hasattr(f, "grad_async") and isinstance(x, torch.Tensor) and x.is_cuda


_BURG_SIMPLEX_HOOKS = ("div_prox_map", "prox_map", "_prox", "divergence", "extra_Psi")


def _can_one_wait(f, h, x, checkdiv):
    """ABPG_gain runs its line-search trials through accbpg_dopt_burg_trial (DOptimalObj.one_wait_trials, on by
    default) on this package's D-optimal objective evaluating directly -- no Gram reuse, no gradients started ahead, no
    memo, not a shard, not a batch instance -- with the Burg simplex kernel, device iterates and the value test.  A
    native trial passes by the Python methods of f and h, so an objective or a kernel whose methods were overridden in
    a subclass or wrapped on the instance keeps the stepwise loop, which calls them."""
    if checkdiv or not isinstance(f, DOptimalObj) or not f._one_wait_ok():
        return False
    if type(h) is not BurgEntropySimplex or any(name in vars(h) for name in _BURG_SIMPLEX_HOOKS):
        return False
    return isinstance(x, torch.Tensor) and x.is_cuda and x.device == f.device


def _value_end(f, pending):
    kind, payload = pending
    return f.value_wait(payload) if kind == "ticket" else payload


def _stamp(f, pending, t_start, t_known):
    """T[k]: seconds from the start of the run to the moment F[k] = f(x) was known, as the reference stamps
    it right after that evaluation (accbpg/algorithms.py:135-137, 347-349).  `t_known` is the host clock when
    the value came back on the solver's stream; a value that ran beside the gradient evaluation was known
    earlier than the clock read that follows both by the lead the device reports."""
    if pending[0] == "ticket":
        return time.time() - t_start - f.value_lead_seconds()
    return t_known - t_start


def _drain(gen):
    """Run a step generator to completion and return its result."""
    while True:
        try:
            next(gen)
        except StopIteration as stop:
            return stop.value


def BPG(f, h, L, x0, maxitrs, epsilon=1e-14, linesearch=True, ls_ratio=1.2,
        verbose=True, verbskip=1):
    """Bregman proximal gradient method (accbpg/algorithms.py:11-72).

    Returns (x, F, Ls, T).  F[k] is the objective at the iterate *before* update k
    (:47), so the returned x is one step past F[-1]; L is carried between iterations
    and divided by ls_ratio before each backtracking search (:51)."""
    return _drain(BPG_steps(f, h, L, x0, maxitrs, epsilon, linesearch, ls_ratio, verbose, verbskip))


def BPG_steps(f, h, L, x0, maxitrs, epsilon=1e-14, linesearch=True, ls_ratio=1.2,
              verbose=True, verbskip=1):
    """Generator form of BPG: yields k after each outer iteration, returns BPG's tuple."""
    if verbose:
        print("\nBPG_LS method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)         Lk       time")

    t_start = time.time()
    run = _BPGRun(L, maxitrs, epsilon, linesearch, ls_ratio)

    x, as_numpy = to_dev(x0)
    x = x.clone()
    for k in range(maxitrs):
        fx, g = f.func_grad(x)
        run.begin(k, fx + h.extra_Psi(x), time.time() - t_start)

        trial = h.div_prox_map(x, g, run.L)
        while linesearch:
            lin, dist, _ = _divergences(h, g, trial, x, None, None)
            if run.accepts(f(trial), fx, lin, dist):            # algorithms.py:53
                break
            trial = h.div_prox_map(x, g, run.L)
        x = trial

        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:6.1f}".format(k, run.F[k], run.L, run.T[k]))

        if run.finish():                                        # algorithms.py:66
            break
        yield k

    return run.result(from_dev(x, as_numpy))


def ABPG(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=False,
         restart=False, restart_rule='g', verbose=True, verbskip=1):
    """Accelerated BPG with fixed triangle-scaling exponent (accbpg/algorithms.py:94-180).
    Returns (x, F, G, T)."""
    return _drain(ABPG_steps(f, h, L, x0, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule,
                             verbose, verbskip))


def ABPG_steps(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=False,
               restart=False, restart_rule='g', verbose=True, verbskip=1):
    """Generator form of ABPG: yields k after each outer iteration, returns ABPG's tuple."""
    if verbose:
        print("\nABPG method for minimize_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       theta" +
              "        TSG       D(x+,y)     D(z+,z)     time")

    t_start = time.time()
    run = _ABPGRun(L, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule)

    x, as_numpy = to_dev(x0)
    x = x.clone()
    z = x.clone()
    xcombo = None
    for k in range(maxitrs):
        pending = _value_begin(f, x, xcombo)                    # :135 (runs beside the gradient below)
        t_known = time.time()

        z_prev, x_prev = z, x
        theta = run.begin(k)                                    # :142-145

        y = vec_axpby(1 - theta, x, theta, z_prev)              # :147
        if _lin(f):
            g = f.func_grad_combo(y, (1 - theta, x_prev, theta, z_prev), 1)
        else:
            g = f.gradient(y)                                   # :148
        run.record(_value_end(f, pending) + h.extra_Psi(x_prev), _stamp(f, pending, t_start, t_known))   # :136-137
        z = h.div_prox_map(z_prev, g, run.prox_coef())          # :149
        x = vec_axpby(1 - theta, x, theta, z)                   # :150
        if _lin(f):
            f.ensure_gram(z)                                    # the one O(m^2 n) product of this iteration
            xcombo = (1 - theta, x_prev, theta, z)

        _, dxy, dzz = _divergences(h, None, x, y, z, z_prev)    # :153-154
        Gdr = run.divergences(dxy, dzz)                         # :155
        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:10.3e}  {5:10.3e}  {6:6.1f}".format(
                k, run.F[k], theta, Gdr, dxy, dzz, run.T[k]))

        restarted, stop = run.finish(vec_dot_diff(g, x, x_prev) if run.needs_dot() else None)   # :165-171
        if restarted:
            z = x

        if stop:                                                # :174
            break
        yield k

    return run.result(from_dev(x, as_numpy))


def ABPG_gain(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, G0=1,
              ls_inc=1.2, ls_dec=1.2, theta_eq=True, checkdiv=False,
              restart=False, restart_rule='g', verbose=True, verbskip=1):
    """Accelerated BPG with gain adaption (accbpg/algorithms.py:295-420).
    Returns (x, F, Gain, Gdiv, Gavg, T).  The reference's quirks are kept: see ``solver_runs._GainRun``."""
    return _drain(ABPG_gain_steps(f, h, L, x0, gamma, maxitrs, epsilon, G0, ls_inc, ls_dec, theta_eq,
                                  checkdiv, restart, restart_rule, verbose, verbskip))


def ABPG_gain_steps(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, G0=1,
                    ls_inc=1.2, ls_dec=1.2, theta_eq=True, checkdiv=False,
                    restart=False, restart_rule='g', verbose=True, verbskip=1):
    """Generator form of ABPG_gain: yields k after each outer iteration, returns its tuple.

    With DOptimalObj.one_wait_trials (the default, see ``_can_one_wait``) a line-search trial is one native call with
    one wait, and F[k] is answered inside the first trial of iteration k: T[k] is then stamped when F[k] is known on
    the host, which is at that trial's wait.  A trial that has to be replayed stepwise has dropped the value record, so
    an F[k] that rode in it is evaluated in full: the same number, one less in ``values_reused``."""
    if verbose:
        print("\nABPG_gain method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       theta         Gk" +
              "         TSG       D(x+,y)     D(z+,z)      Gavg       time")

    t_start = time.time()
    run = _GainRun(L, gamma, maxitrs, epsilon, G0, ls_inc, ls_dec, theta_eq, checkdiv, restart, restart_rule)

    x, as_numpy = to_dev(x0)
    x = x.clone()
    z = x.clone()
    xcombo = None
    for k in range(maxitrs):
        z_prev, x_prev = z, x
        run.begin(k)                                            # :358

        # a whole trial per call and one wait (DOptimalObj.one_wait_trials); where the accepting test left its value
        # record at x (DOptimalObj.reuse_values) F[k] rides in the first trial, which answers it from that record
        one_wait = _can_one_wait(f, h, x_prev, checkdiv)
        pending = None if one_wait and f.value_recorded(x_prev) else _value_begin(f, x, xcombo)   # :347 (beside the first gradient)
        t_known = time.time()
        fk_due = True

        ahead = _can_speculate(f, x_prev, checkdiv)
        started = None                                          # (y, ticket) of a gradient evaluation started ahead
        while True:                                             # :361
            theta = run.trial()                                 # :362-367
            done = None
            if one_wait:                                        # :369-378 and f(x) of :387, None: replay it stepwise
                done = f.trial(x_prev, z_prev, theta, run.prox_coef(), h.eps, fk_due and pending is None)
            if fk_due and pending is None and (done is None or not done[4].fk_answered):
                # F[k] was not answered in the trial (x changed in place under its record): evaluate it
                pending = _value_begin(f, x_prev, xcombo)
                t_known = time.time()
            if done is not None:
                y, g, z, x, res = done
                fy = res.fy
                h.last_info = (res.prox_info[0], res.prox_info[1])
            elif started is not None:
                y, ticket = started                             # the point and the evaluation of this very trial
                started = None
                fy, g = f.grad_wait(ticket)
            else:
                y = vec_axpby(1 - theta, x_prev, theta, z_prev)  # :369
                if _lin(f):
                    fy, g = f.func_grad_combo(y, (1 - theta, x_prev, theta, z_prev), 2)
                else:
                    fy, g = f.func_grad(y)                      # :371
            if fk_due:                                          # :348-349
                if pending is None:                             # it came with the trial: known at the trial's wait
                    run.record(res.fk + h.extra_Psi(x_prev), time.time() - t_start)
                else:
                    run.record(_value_end(f, pending) + h.extra_Psi(x_prev), _stamp(f, pending, t_start, t_known))
                    pending = None
                fk_due = False
            if done is not None:
                lin, dxy, dzz = np.float64(res.lin), np.float64(res.dxy), np.float64(res.dzz)
            else:
                z = h.div_prox_map(z_prev, g, run.prox_coef())  # :373
                x = vec_axpby(1 - theta, x_prev, theta, z)      # :374
                if _lin(f):
                    f.ensure_gram(z)                            # the one O(m^2 n) product of this pass
                    xcombo = (1 - theta, x_prev, theta, z)

                lin, dxy, dzz = _divergences(h, g, x, y, z, z_prev)  # :377-378 and the dot of :387

            verdict = run.divergences(lin, dxy, dzz)            # :379-385
            if verdict == BREAK:                                # (a value the trial computed is dropped)
                break
            if verdict == NEEDS_VALUE:
                if ahead and run.failed < run.retries_before:
                    # the previous iteration failed this trial too: the next trial's gradient (a function of host
                    # scalars and of x_1, z_1 only) goes out on the side stream beside the value test below
                    theta_next = run.theta_for(run.G * ls_inc)
                    y_next = vec_axpby(1 - theta_next, x_prev, theta_next, z_prev)
                    started = (y_next, f.grad_async(y_next))
                if done is not None:
                    f.calls["value"] += 1                       # f(x) came with the trial
                    fx = res.fx
                else:
                    fx = _value(f, x, xcombo)
                verdict = run.value(fx, fy)                     # :387
            if verdict == ACCEPT:
                if started is not None:
                    f.grad_drop(started[1])                     # the trial passed: not needed
                    started = None
                break

        restarted, stop = run.finish(vec_dot_diff(g, x, x_prev) if run.needs_dot() else None)   # :395-409
        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:10.3e}  {5:10.3e}  {6:10.3e}  {7:10.3e}  {8:6.1f}".format(
                k, run.F[k], theta, run.G, run.Gdr, dxy, dzz, run.Gavg[k], run.T[k]))
        if restarted:
            z = x

        if stop:                                                # :412
            break
        yield k

    return run.result(from_dev(x, as_numpy))


def ABPG_expo(f, h, L, x0, gamma0, maxitrs, epsilon=1e-14, delta=0.2,
              theta_eq=True, checkdiv=False, Gmargin=10, restart=False,
              restart_rule='g', verbose=True, verbskip=1):
    """Accelerated BPG with exponent adaption (accbpg/algorithms.py:183-292).
    Returns (x, F, Gamma, G, T).  One gradient at y per outer iteration (:245); the inner loop
    lowers gamma by delta while its test fails and gamma > 1 (:262-265); the restart test has no
    k > 0 guard (:276-282)."""
    return _drain(ABPG_expo_steps(f, h, L, x0, gamma0, maxitrs, epsilon, delta, theta_eq, checkdiv, Gmargin,
                                  restart, restart_rule, verbose, verbskip))


def ABPG_expo_steps(f, h, L, x0, gamma0, maxitrs, epsilon=1e-14, delta=0.2,
                    theta_eq=True, checkdiv=False, Gmargin=10, restart=False,
                    restart_rule='g', verbose=True, verbskip=1):
    """Generator form of ABPG_expo: yields k after each outer iteration, returns its tuple."""
    if verbose:
        print("\nABPG_expo method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       theta       gamma" +
              "        TSG       D(x+,y)     D(z+,z)     time")

    t_start = time.time()
    run = _ExpoRun(L, gamma0, maxitrs, epsilon, delta, theta_eq, checkdiv, Gmargin, restart, restart_rule)

    x, as_numpy = to_dev(x0)
    x = x.clone()
    z = x.clone()
    for k in range(maxitrs):
        Fk = f(x) + h.extra_Psi(x)                              # :231-232
        z_prev, x_prev = z, x
        theta = run.begin(k)                                    # :238-241
        run.record(Fk, time.time() - t_start)

        y = vec_axpby(1 - theta, x_prev, theta, z_prev)         # :243
        fy, g = f.func_grad(y)                                  # :245

        while True:                                             # :248
            z = h.div_prox_map(z_prev, g, run.prox_coef())      # :249
            x = vec_axpby(1 - theta, x_prev, theta, z)          # :250
            lin, dxy, dzz = _divergences(h, g, x, y, z, z_prev)  # :253-254 and the dot of :260
            verdict = run.divergences(lin, dxy, dzz)            # :255-258
            if verdict == NEEDS_VALUE:
                verdict = run.value(f(x), fy)                   # :260
            if verdict == ACCEPT:                               # :262-265
                break

        restarted, stop = run.finish(vec_dot_diff(g, x, x_prev) if run.needs_dot() else None)   # :267-282
        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:10.3e}  {5:10.3e}  {6:10.3e}  {7:6.1f}".format(
                k, run.F[k], theta, run.gamma, run.Gdr, dxy, dzz, run.T[k]))
        if restarted:
            z = x

        if stop:                                                # :285
            break
        yield k

    return run.result(from_dev(x, as_numpy))


def ABDA(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=True,
         verbose=True, verbskip=1):
    """Accelerated Bregman dual averaging (accbpg/algorithms.py:423-514).  Returns (x, F, G, T).
    gavg accumulates theta^(1-gamma) * g (:483), z = prox_map(gavg/csum, L/csum) (:485)."""
    return _drain(ABDA_steps(f, h, L, x0, gamma, maxitrs, epsilon, theta_eq, verbose, verbskip))


def ABDA_steps(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=True,
               verbose=True, verbskip=1):
    """Generator form of ABDA: yields k after each outer iteration, returns ABDA's tuple."""
    if verbose:
        print("\nABDA method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       theta" +
              "        TSG       D(x+,y)     D(z+,z)     time")

    t_start = time.time()
    run = _ABDARun(L, gamma, maxitrs, epsilon, theta_eq)

    x, as_numpy = to_dev(x0)
    x = x.clone()
    z = x.clone()
    gavg = torch.zeros_like(x)
    for k in range(maxitrs):
        Fk = f(x) + h.extra_Psi(x)                              # :465-466
        z_prev, x_prev = z, x
        theta = run.begin(k)                                    # :472-475
        run.record(Fk, time.time() - t_start)

        y = vec_axpby(1 - theta, x_prev, theta, z_prev)         # :477
        g = f.gradient(y)                                       # :478
        wgt, csum, Lc = run.weight()                            # :480
        gavg = vec_axpby(1.0, gavg, wgt, g)                     # :479  (1.0*gavg is exact)
        z = h.prox_map(vec_div_scalar(gavg, csum), Lc)          # :481
        x = vec_axpby(1 - theta, x_prev, theta, z)              # :482

        _, dxy, dzz = _divergences(h, None, x, y, z, z_prev)    # :485-486
        Gdr = run.divergences(dxy, dzz)
        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:10.3e}  {4:10.3e}  {5:10.3e}  {6:6.1f}".format(
                k, run.F[k], theta, Gdr, dxy, dzz, run.T[k]))

        _, stop = run.finish()
        if stop:                                                # :508
            break
        yield k

    return run.result(from_dev(x, as_numpy))


# ---------------------------------------------------------------------------------------------------------------
# Inexact-oracle accelerated methods (accbpg/algorithms.py:593-777).  One line-search try is a handful of length-n
# passes around two or three evaluations of f; at the drivers' size those cost launches and read-backs, not
# bandwidth, so the extrapolated point and the two numbers of the test come from one kernel (combine_ls_terms)
# and AIBM's accumulated-gradient prox from another (BurgEntropySimplex.prox_map_acc).  FUSED_INEXACT = False
# composes the same loops from the package's public kernels (same elementwise rounding); tools/inexact_rate.py
# times both.  Where the reference evaluates f.gradient(x) and f(x) at one point, func_grad(x, 2) gives both.
# ---------------------------------------------------------------------------------------------------------------
FUSED_INEXACT = True


def _fusable(h):
    return FUSED_INEXACT and isinstance(h, (BurgEntropy, SquaredL2Norm))


def _combine(h, a, u, b, v, c, g=None, x=None):
    """(w, <g, w-x>, D_h(w, x)) with w = (a*u + b*v)/c; the two numbers only when x is given."""
    if _fusable(h):
        return combine_ls_terms(h, a, u, b, v, c, g, x)
    w = vec_axpby(a, u, b, v)
    if c != 1:
        w = vec_div_scalar(w, c)
    if x is None:
        return w, None, None
    lin, dist, _ = _divergences(h, g, w, x, None, None)
    return w, lin, dist


def _doubled(L):
    """L*2 of a failed try.  The reference's AIBM and AdaptFGM have no way out once L has doubled to infinity (their
    test is false from then on); here all three methods stop as its UniversalGM does (:759-760)."""
    L = L * 2
    if L is None or not math.isfinite(L):
        raise ValueError("L cannot be None or infinity")
    return L


def AIBM(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, verbose=True, noise=0, verbskip=1):
    """Adaptive intermediate Bregman method with an inexact oracle (accbpg/algorithms.py:593-658).
    Returns (x, F, G, T).

    Quirks kept: x0 gives the length only, the run starts from ones * h.prox_map(zeros, 1) (:604); the first search
    tests with + epsilon + delta (:611), the others with + delta; G[0] = L and the rest of G stays zero; the stopping
    threshold is 1e-9, not epsilon (:652); a rejected try adds alpha*grad to xi_grad and subtracts it again (:630,
    :636), which does not restore its bits; the returned x is the last extrapolated point, where F[k] was taken.
    delta = get_random_float(noise) is drawn once before the first search and once per k."""
    return _drain(AIBM_steps(f, h, L, x0, gamma, maxitrs, epsilon, verbose, noise, verbskip))


def AIBM_steps(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, verbose=True, noise=0, verbskip=1):
    """Generator form of AIBM: yields k after each outer iteration, returns AIBM's tuple."""
    if verbose:
        print("\nAIBM method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       L       time")

    t_start = time.time()
    F = np.zeros(maxitrs)
    G = np.zeros(maxitrs)
    T = np.zeros(maxitrs)
    p = 2

    x0d, as_numpy = to_dev(x0)
    x = z = h.prox_map(torch.zeros(x0d.shape[0], dtype=torch.float64, device=x0d.device), 1)   # :604 (ones * it is exact)

    delta = get_random_float(noise)
    fx, g = f.func_grad(x, flag=2)
    y = h.prox_map(g, 1)                                        # :610-611 do not depend on L: evaluated once
    lin, dist, _ = _divergences(h, g, y, x, None, None)
    fy = f(y)
    while True:
        alpha = 1 / L
        if fy <= fx + lin + L * dist + epsilon + delta:
            break
        L = _doubled(L)

    B = A = alpha
    xi_grad = vec_axpby(alpha, g, 0.0, g)                       # :616 alpha * f.gradient(x), the gradient held already

    F[0] = fx + h.extra_Psi(x)
    G[0] = L
    T[0] = time.time() - t_start

    acc_prox = FUSED_INEXACT and isinstance(h, BurgEntropySimplex)
    k = 0
    for k in range(1, maxitrs):
        L /= 2
        delta = get_random_float(noise)
        while True:
            alpha = (1 / L) * (1 + k / (2 * p)) ** ((p - 1) * (gamma - 1))
            B = (L * alpha ** gamma) ** (1 / (gamma - 1))
            x = vec_axpby(alpha / B, z, 1 - alpha / B, y)       # :628
            fx, grad_x = f.func_grad(x, flag=2)                 # :629 and :633
            if acc_prox:
                xi_grad, z_k = h.prox_map_acc(xi_grad, alpha, grad_x)      # :630-631
            else:
                xi_grad = vec_axpby(1.0, xi_grad, alpha, grad_x)
                z_k = h.prox_map(xi_grad, 1)
            w, lin, dist = _combine(h, alpha / B, z_k, 1 - alpha / B, y, 1, grad_x, x)   # :632 and the terms of :634
            if f(w) <= fx + lin + L * dist + delta:
                break
            xi_grad = vec_axpby(1.0, xi_grad, -alpha, grad_x)   # :636
            L = _doubled(L)

        F[k] = fx + h.extra_Psi(x)
        T[k] = time.time() - t_start

        A += alpha
        y = vec_axpby(B / A, w, 1 - B / A, y)                   # :644
        z = z_k

        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:6.1f}".format(k, F[k], L, T[k]))

        if abs(F[k] - F[k - 1]) < 1e-9:                         # :652
            break
        yield k

    return from_dev(x, as_numpy), F[0:k + 1], G[0:k + 1], T[0:k + 1]


def AdaptFGM(f, h, L, x0, maxitrs, epsilon=1e-14, verbose=True, noise=0, verbskip=1):
    """Adaptive fast gradient method with an inexact oracle (accbpg/algorithms.py:661-714).  Returns (x_k, F, G, T).

    Quirks kept: x_k, y and u_k all start at ones(x0.shape), off the simplex, and F[0] is taken there (:671-676);
    f(x_k), not f(y), enters every try (:691-692); the linear term is sum(g_y*(x - y)).  f(x_k) is the value held from
    the evaluation that accepted x_k (the same number)."""
    return _drain(AdaptFGM_steps(f, h, L, x0, maxitrs, epsilon, verbose, noise, verbskip))


def AdaptFGM_steps(f, h, L, x0, maxitrs, epsilon=1e-14, verbose=True, noise=0, verbskip=1):
    """Generator form of AdaptFGM: yields k after each outer iteration, returns AdaptFGM's tuple."""
    if verbose:
        print("\nAdaptFGM method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       L       time")

    t_start = time.time()
    F = np.zeros(maxitrs)
    G = np.zeros(maxitrs)
    T = np.zeros(maxitrs)

    x0d, as_numpy = to_dev(x0)
    x_k = u_k = torch.ones(x0d.shape, dtype=torch.float64, device=x0d.device)
    A_k = 0

    fxk, g = f.func_grad(x_k, flag=2)

    F[0] = fxk + h.extra_Psi(x_k)
    G[0] = L
    T[0] = time.time() - t_start

    k = 0
    for k in range(1, maxitrs):
        L /= 2
        delta = get_random_float(noise)
        while True:
            alpha = (1 + math.sqrt(1 + 4 * L * A_k)) / (2 * L)
            A = L * alpha ** 2
            y, _, _ = _combine(h, alpha, u_k, A_k, x_k, A)      # :686
            g_y = f.gradient(y)
            u = h.div_prox_map(u_k, vec_axpby(alpha, g_y, 0.0, g_y), 1)
            x, lin, dist = _combine(h, alpha, u, A_k, x_k, A, g_y, y)      # :689 and the terms of :692
            fx = f(x)
            if fx <= fxk + lin + L * dist + delta:
                A_k = A
                u_k = u
                x_k = x
                fxk = fx
                break
            L = _doubled(L)

        F[k] = fxk + h.extra_Psi(x_k)
        G[k] = L
        T[k] = time.time() - t_start

        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:6.1f}".format(k, F[k], L, T[k]))

        if abs(F[k] - F[k - 1]) < epsilon:
            break
        yield k

    return from_dev(x_k, as_numpy), F[0:k + 1], G[0:k + 1], T[0:k + 1]


def UniversalGM(f, h, L, x0, maxitrs, epsilon=1e-14, verbose=True, noise_level=0, verbskip=1):
    """Universal gradient method with a noisy oracle (accbpg/algorithms.py:717-777).  Returns (x_k, F, G, T).

    Quirks kept: x0 feeds F[0] only (the first y is u_k/(L*alpha) with u_k = ones, since A_k = 0); one scalar
    noise = np.random.rand()*noise_level is drawn per k when noise_level > 0 and added to every component of the
    gradient and to f(y)."""
    return _drain(UniversalGM_steps(f, h, L, x0, maxitrs, epsilon, verbose, noise_level, verbskip))


def UniversalGM_steps(f, h, L, x0, maxitrs, epsilon=1e-14, verbose=True, noise_level=0, verbskip=1):
    """Generator form of UniversalGM: yields k after each outer iteration, returns UniversalGM's tuple."""
    if verbose:
        print("\nUniversalGM method for min_{x in C} F(x) = f(x) + Psi(x)")
        print("     k      F(x)       L       time")

    t_start = time.time()
    F = np.zeros(maxitrs)
    G = np.zeros(maxitrs)
    T = np.zeros(maxitrs)

    x0d, as_numpy = to_dev(x0)
    x_k = x0d.clone()
    fxk = f(x_k)
    F[0] = fxk + h.extra_Psi(x_k)
    G[0] = L
    T[0] = time.time() - t_start

    A_k = 0
    ones = torch.ones(x0d.shape, dtype=torch.float64, device=x0d.device)
    u_k = ones

    k = 0
    for k in range(1, maxitrs):
        noise = np.random.rand() * noise_level if noise_level > 0 else 0

        L /= 2
        while True:
            alpha = (1 + math.sqrt(1 + 4 * L * A_k)) / (2 * L)
            A = L * alpha ** 2
            y, _, _ = _combine(h, alpha, u_k, A_k, x_k, A)      # :744
            fy, g_y = f.func_grad(y, flag=2)                    # :745 and :750
            if noise_level > 0:
                g_y = vec_axpby(1.0, g_y, noise, ones)          # g_y += noise
            u = h.div_prox_map(u_k, vec_axpby(alpha, g_y, 0.0, g_y), 1)
            x, lin, dist = _combine(h, alpha, u, A_k, x_k, A, g_y, y)      # :748 and the terms of :753

            fy += noise
            fx = f(x)
            if fx <= fy + lin + L * dist:
                A_k = A
                u_k = u
                x_k = x
                fxk = fx
                break
            L = _doubled(L)

        F[k] = fxk + h.extra_Psi(x_k)
        G[k] = L
        T[k] = time.time() - t_start

        if verbose and k % verbskip == 0:
            print("{0:6d}  {1:10.3e}  {2:10.3e}  {3:6.1f}".format(k, F[k], L, T[k]))

        if abs(F[k] - F[k - 1]) < epsilon:
            break
        yield k

    return from_dev(x_k, as_numpy), F[0:k + 1], G[0:k + 1], T[0:k + 1]
