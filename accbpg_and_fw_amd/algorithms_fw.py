"""Frank-Wolfe with a step length taken from the Bregman divergence to the LMO vertex, on device
vectors or n x r matrices (behaviour of accbpg/algorithms_fw.py:6-75; used with ``lmo_simplex`` on the
D-optimal objective as in frank_wolfe_wtih_rs/ex_Dopt_design.py:17-18, and with the ball LMOs on the
SymNMF objective as in parameters_free_fw/ipynb/ex_SymNMF.ipynb), and Frank-Wolfe with the classical
step 2/(k+2) (accbpg/algorithms_fw.py:210-247).

Written like the other solvers of this package: a step generator that the public function drains,
preallocated traces cut to the iterations that ran, and one fused launch for the slope <g, s - x> and
the divergence D(s, x) when h is the Burg kernel.
"""
from __future__ import annotations

import math
import time

import numpy as np

from .algorithms import _divergences, _drain
from .functions import SquaredL2Norm, from_dev, to_dev, vec_axpby, vec_dot
from .functions_lmo import _Lmo, fw_direction
from .solver_runs import _LogLinearRun, _LogOnlyRun, _ShortestStepRun

_SLOPE_FLOOR = 1e-6     # stand-in for a vanishing divergence, and the band of slopes treated as zero


def _check_options(L, epsilon, ls_ratio):
    for bad, message in ((ls_ratio < 1, "ls_ratio must be >= 1"),
                         (L <= 0, "Initial L must be positive"),
                         (epsilon <= 0, "epsilon must be positive")):
        if bad:
            raise ValueError(message)


def _step_length(slope, L, dist, gamma):
    """min((-slope / (2 L D))^(1/(gamma-1)), 1): minimiser of the upper model along s - x."""
    return min((-slope / (2 * L * dist)) ** (1 / (gamma - 1)), 1.0)


def FW_alg_div_step(f, h, L, x0, maxitrs, gamma, lmo, epsilon=1e-14, linesearch=True, ls_ratio=2,
                    verbose=True, verbskip=1):
    """Returns (x, F, Ls, T).  Each iteration moves from x towards the vertex s = lmo(grad f(x)) by
    the step length above; with `linesearch` the constant L is first divided by ls_ratio and then
    multiplied back until f(x+) <= f(x) + a*slope + a^gamma * L * D(s, x).

    On the D-optimal objective with the Burg kernel and ``lmo_simplex``, ``D_opt_FW_div_step`` (D_opt_alg.py) runs the
    same iteration at O(mn) per step on rank-one updates of the inverse Gram matrix; this function does not dispatch to
    it."""
    return _drain(FW_alg_div_step_steps(f, h, L, x0, maxitrs, gamma, lmo, epsilon, linesearch, ls_ratio,
                                        verbose, verbskip))


def FW_alg_div_step_steps(f, h, L, x0, maxitrs, gamma, lmo, epsilon=1e-14, linesearch=True, ls_ratio=2,
                          verbose=True, verbskip=1):
    """Generator form: yields k after each outer iteration, returns FW_alg_div_step's tuple."""
    _check_options(L, epsilon, ls_ratio)
    if verbose:
        print("\nFW adaptive algorithm")
        print("     k      F(x)         Lk       time")

    t_start = time.time()
    F = np.zeros(maxitrs)
    Ls = np.zeros(maxitrs)
    T = np.zeros(maxitrs)

    point, as_numpy = to_dev(x0)
    point = point.clone()
    done = 0
    for k in range(maxitrs):
        value, grad = f.func_grad(point)
        F[k] = value + h.extra_Psi(point)
        T[k] = time.time() - t_start

        vertex = lmo(grad)
        slope, dist, _ = _divergences(h, grad, vertex, point, None, None)     # <g, s - x> and D(s, x)
        dist = dist if dist != 0 else _SLOPE_FLOOR
        if 0 < slope <= _SLOPE_FLOOR:
            slope = 0.0
        if slope > 0:
            raise ValueError("grad_d_prod must be non-positive")
        towards = vec_axpby(1.0, vertex, -1.0, point)                          # s - x, one rounding

        if linesearch:
            L = L / ls_ratio
        while True:
            a = _step_length(slope, L, dist, gamma)
            trial = vec_axpby(1.0, point, a, towards)                          # x + a*(s - x)
            if not linesearch:
                break
            assert not math.isinf(L), "L is infinite"
            if f.func_grad(trial, flag=0) <= value + a * slope + a ** gamma * L * dist:
                break
            L = L * ls_ratio

        point = trial
        Ls[k] = L
        done = k + 1
        if verbose and k % verbskip == 0:
            print(f"{k:6d}  {F[k]:10.3e}  {L:10.3e}  {T[k]:6.1f}")
        if k > 0 and abs(F[k] - F[k - 1]) < epsilon:
            break
        yield k

    return from_dev(point, as_numpy), F[:done], Ls[:done], T[:done]


def FW_alg_descent_step(f, h, x0, maxitrs, lmo, epsilon=1e-14, verbose=True, verbskip=1):
    """Returns (x, F, T, G) with G all zeros, as the reference does.  Iteration k >= 1 moves x by 2/(k+2) towards
    s = lmo(grad f(x)) and stops on |F[k] - F[k-1]| < epsilon or ||grad f(x)|| < epsilon.  With maxitrs = 1 the
    reference fails (UnboundLocalError on k); this returns the single evaluation at x0.

    On the D-optimal objective with ``lmo_simplex``, ``D_opt_FW_descent_step`` (D_opt_alg.py) runs the same iteration at
    O(mn) per step; this function does not dispatch to it."""
    return _drain(FW_alg_descent_step_steps(f, h, x0, maxitrs, lmo, epsilon, verbose, verbskip))


def FW_alg_descent_step_steps(f, h, x0, maxitrs, lmo, epsilon=1e-14, verbose=True, verbskip=1):
    """Generator form: yields k after each iteration, returns FW_alg_descent_step's tuple."""
    if verbose:
        print("\nFW descent step size algorithm")
        print("     k      F(x)         alpha_k       time")

    t_start = time.time()
    F = np.zeros(maxitrs)
    G = np.zeros(maxitrs)
    T = np.zeros(maxitrs)

    point, as_numpy = to_dev(x0)
    point = point.clone()
    value, grad = f.func_grad(point)
    F[0] = value + h.extra_Psi(point)
    T[0] = time.time() - t_start

    k = 0
    for k in range(1, maxitrs):
        vertex = lmo(grad)
        towards = vec_axpby(1.0, vertex, -1.0, point)                          # d = s - x
        alpha = 2 / (k + 2)
        point = vec_axpby(1.0, point, alpha, towards)                          # x + alpha*d

        value, grad = f.func_grad(point)
        F[k] = value + h.extra_Psi(point)
        T[k] = time.time() - t_start

        if verbose and (k % verbskip == 0 or k == 1):
            print(f"{k:6d}  {F[k]:10.3e}  {alpha:10.3e}  {T[k]:6.1f}")

        if abs(F[k] - F[k - 1]) < epsilon or math.sqrt(vec_dot(grad, grad)) < epsilon:
            break
        yield k

    return from_dev(point, as_numpy), F[:k + 1], T[:k + 1], G[:k + 1]


# ---------------------------------------------------------------------------------------------------------------
# Frank-Wolfe for (L0, L1)-smooth objectives (accbpg/algorithms_fw.py:78-207, :250-349, :352-453).  The host
# decisions are the run objects of solver_runs.py; this file moves the vectors.
#
# One iteration of the generic composition is a func_grad (two passes over the data), the oracle, s - x, three inner
# products with a read-back each, and a value per trial (one pass each).  Two things shorten it:
#   fused   with an oracle of functions_lmo.py the direction step is one call and one read-back (fw_direction): s, d,
#           <g, g>, <g, d>, <d, d>, every entry and every sum with the bits of the composition, so the run is the same
#           run bit for bit;
#   carry   with an objective that has line_begin / line_value / line_accept / func_grad_carried (LogisticRegression)
#           the margins are carried along the segment: one pass for A d, every trial O(m), and the next iteration's
#           value and gradient from the accepted margins, with a full func_grad every ``refresh`` iterations.  The
#           carried margins fma(a, (A d)_i, (A x)_i) differ from A (x + a d) by rounding, so this run is not bit for
#           bit the other one; it is opt-in.
# ---------------------------------------------------------------------------------------------------------------
_LINE_METHODS = ("line_begin", "line_value", "line_accept", "func_grad_carried")


def _direction(lmo, h, grad, point, fused, want_div):
    """(d, sum g^2, <g, d>, sum d^2, D(s, x) or None) at the gradient ``grad`` of ``point``."""
    if fused and isinstance(lmo, _Lmo):
        vertex, towards, gg, slope, dd, _, _ = fw_direction(lmo, grad, point)
        div = None
        if want_div:
            div = 0.5 * dd if type(h) is SquaredL2Norm else h.divergence(vertex, point)
        return towards, gg, slope, dd, div
    vertex, _ = to_dev(lmo(grad))
    vertex = vertex.reshape(point.shape)
    towards = vec_axpby(1.0, vertex, -1.0, point)                              # s - x, one rounding
    div = h.divergence(vertex, point) if want_div else None
    return (towards, np.float64(vec_dot(grad, grad)), np.float64(vec_dot(grad, towards)),
            np.float64(vec_dot(towards, towards)), div)


def _l0l1_steps(run, f, h, x0, maxitrs, lmo, verbose, verbskip, fused, carry, refresh, want_div, row):
    """The iteration the three solvers share; ``run`` decides, ``row(k)`` prints."""
    t_start = time.time()
    point, as_numpy = to_dev(x0)
    point = point.clone()
    line = bool(carry) and all(hasattr(f, name) for name in _LINE_METHODS)
    assert refresh >= 1, "refresh must be at least 1"
    for k in range(maxitrs):
        if line and k % refresh != 0:
            value, grad = f.func_grad_carried(2)
            grad = grad.reshape(point.shape)
        else:
            value, grad = f.func_grad(point)
        run.begin(k, value, value + h.extra_Psi(point), time.time() - t_start)

        towards, gg, slope, dd, div = _direction(lmo, h, grad, point, fused, want_div)
        if not run.direction(np.sqrt(gg), slope, div if want_div else np.sqrt(dd)):
            break                                                              # d = 0: nothing to move along
        if line:
            f.line_begin(towards)
        while True:
            a = run.step()
            if not line:
                trial = vec_axpby(1.0, point, a, towards)                      # x + a*d
            if not run.linesearch:
                break
            if run.accepts(f.line_value(a) if line else f.func_grad(trial, flag=0)):
                break
        if line:
            trial = vec_axpby(1.0, point, a, towards)
            f.line_accept(a)
        point = trial

        stop = run.finish()
        if verbose and k % verbskip == 0:
            print(row(k))
        if stop:
            break
        yield k

    return run.result(from_dev(point, as_numpy))


def FW_alg_L0_L1_shortest_step(f, h, L0, L1, x0, maxitrs, gamma, lmo, epsilon=1e-14, linesearch=True, ls_ratio=2,
                               verbose=True, verbskip=1, *, fused=True, carry=False, refresh=64):
    """Returns (x, F, Ls, T) with Ls the constants a_k = L0 + L1 ||grad f(x)||.  The step towards s = lmo(grad f(x)) is
    min((-<g, d> / (a_k D(s, x) e))^(1/(gamma-1)), 1); with `linesearch` L0 and L1 are first divided and then grown in
    turn until f(x+) <= f(x) + a <g, d> + a^gamma (a_k/2) e D(s, x).  D(s, x) == 0 is replaced by 1e-8, so at d = 0 the
    step is 0 and the stop test ends the run one iteration later.

    ``fused``: with an oracle of this package the direction step is one call (fw_direction), bit for bit the
    composition.  ``carry``: with an objective that carries its margins along the segment (LogisticRegression) the
    trials cost O(m) and a full func_grad runs every ``refresh`` iterations only; the values then differ from the
    uncarried run by rounding."""
    return _drain(FW_alg_L0_L1_shortest_step_steps(f, h, L0, L1, x0, maxitrs, gamma, lmo, epsilon, linesearch, ls_ratio,
                                                   verbose, verbskip, fused=fused, carry=carry, refresh=refresh))


def FW_alg_L0_L1_shortest_step_steps(f, h, L0, L1, x0, maxitrs, gamma, lmo, epsilon=1e-14, linesearch=True, ls_ratio=2,
                                     verbose=True, verbskip=1, *, fused=True, carry=False, refresh=64):
    """Generator form: yields k after each outer iteration, returns FW_alg_L0_L1_shortest_step's tuple."""
    run = _ShortestStepRun(L0, L1, gamma, epsilon, linesearch, ls_ratio)
    if verbose:
        print("\nFW (L0,L1)-smooth algorithm with shortest-step rule")
        print("     k        F(x)          a_k           L0            L1        alpha        time")

    def row(k):
        return (f"{k:6d}   {run.F[k]:10.3e}   {run.Ls[k]:10.3e}   {run.L0:10.3e}   {run.L1:10.3e}   "
                f"{run.alpha:10.3e}   {run.T[k]:6.1f}")

    return (yield from _l0l1_steps(run, f, h, x0, maxitrs, lmo, verbose, verbskip, fused, carry, refresh, True, row))


def _log_row(run):
    return lambda k: (f"{k:6d}   {run.F[k]:10.3e}   {run.Ls[k]:10.3e}   {run.L0:10.3e}   {run.L1:10.3e}   "
                      f"{run.LOG_STEPS[k]:6d}      {run.T[k]:6.1f}")


def FW_l0l1_log_and_linear_step(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon=1e-14, L0_max=None, L1_max=None,
                                linesearch=True, verbose=True, verbskip=50, *, fused=True, carry=False, refresh=64):
    """Returns (x, F, Ls, LOG_STEPS, T).  The step is log(1 - L1 <g, d> / (a_k ||d||)) / (L1 ||d||) when
    L1 ||d|| >= log 2 and L1 (-<g, d>) / (a_k ||d||) otherwise, a_k = L0 + L1 ||grad f(x)||; with `linesearch` both
    constants are divided by ls_ratio and multiplied back (up to L0_max / L1_max, a cap of 0 or None being no cap)
    until f(x+) <= f(x) + a <g, d> + (a_k / L1^2)(e^z - 1 - z), z = L1 a ||d||.  LOG_STEPS starts with a 0 and gains
    one entry per trial, the running count of logarithmic steps.

    At d = 0 the reference divides by zero and goes on with NaN; here the run ends at that iteration with the traces
    so far (F and T hold its entry, Ls does not).  ``fused``, ``carry``, ``refresh``: see FW_alg_L0_L1_shortest_step."""
    return _drain(FW_l0l1_log_and_linear_step_steps(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon, L0_max, L1_max,
                                                    linesearch, verbose, verbskip, fused=fused, carry=carry,
                                                    refresh=refresh))


def FW_l0l1_log_and_linear_step_steps(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon=1e-14, L0_max=None,
                                      L1_max=None, linesearch=True, verbose=True, verbskip=50, *, fused=True,
                                      carry=False, refresh=64):
    """Generator form: yields k after each outer iteration, returns FW_l0l1_log_and_linear_step's tuple."""
    run = _LogLinearRun(L0, L1, ls_ratio, epsilon, L0_max, L1_max, linesearch)
    if verbose:
        print("\nFW L0,L1 smooth logarithmic algorithm")
        print("     k      F(x)         L         L0         L1     log step count       time")
    return (yield from _l0l1_steps(run, f, h, x0, maxitrs, lmo, verbose, verbskip, fused, carry, refresh, False,
                                   _log_row(run)))


def FW_l0l1_log_only(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon=1e-14, L0_max=None, L1_max=None,
                     linesearch=True, verbose=True, verbskip=50, *, fused=True, carry=False, refresh=64):
    """Returns (x, F, Ls, LOG_STEPS, T).  As FW_l0l1_log_and_linear_step, with L1 lifted to log 2 / ||d|| in every
    iteration so that the step is always the logarithmic one, and L0 and L1 grown in turn on a failed test.

    At d = 0 the reference divides by zero and goes on with NaN; here the run ends at that iteration with the traces
    so far (F and T hold its entry, Ls does not).  ``fused``, ``carry``, ``refresh``: see FW_alg_L0_L1_shortest_step."""
    return _drain(FW_l0l1_log_only_steps(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon, L0_max, L1_max, linesearch,
                                         verbose, verbskip, fused=fused, carry=carry, refresh=refresh))


def FW_l0l1_log_only_steps(f, h, L0, L1, x0, maxitrs, lmo, ls_ratio, epsilon=1e-14, L0_max=None, L1_max=None,
                           linesearch=True, verbose=True, verbskip=50, *, fused=True, carry=False, refresh=64):
    """Generator form: yields k after each outer iteration, returns FW_l0l1_log_only's tuple."""
    run = _LogOnlyRun(L0, L1, ls_ratio, epsilon, L0_max, L1_max, linesearch)
    if verbose:
        print("\nFW L0,L1 smooth algorithm with fixed L1")
        print("     k      F(x)         L         L0         L1     log step count       time")
    return (yield from _l0l1_steps(run, f, h, x0, maxitrs, lmo, verbose, verbskip, fused, carry, refresh, False,
                                   _log_row(run)))
