"""The host decisions of BPG / ABPG / ABPG_expo / ABPG_gain / ABDA (accbpg/algorithms.py:11-514), one copy for the single
solvers of ``algorithms.py`` and the lock-step batches of ``batched.py``, as ``_DivStepRun`` / ``_DescentRun`` are for the
Frank-Wolfe solvers.  A run object is one instance's scalars, result arrays and last iteration; it touches no device
and no vector -- the caller does that work and hands over the numbers -- so the CPU tests drive it with NumPy
(tests/test_solver_runs_cpu.py).  Every expression keeps the reference's operation order; the cited lines are its."""
import math

import numpy as np


def solve_theta(theta, gamma, gainratio=1):
    """Newton solve of (1-t)/t^gamma = gainratio/theta^gamma from t = theta, tolerance
    1e-6*theta (accbpg/algorithms.py:75-91).  Pure host scalar arithmetic."""
    ckg = theta ** gamma / gainratio
    cta = theta
    eps = 1e-6 * theta
    phi = cta ** gamma - ckg * (1 - cta)
    while abs(phi) > eps:
        drv = gamma * cta ** (gamma - 1) + ckg
        cta = cta - phi / drv
        phi = cta ** gamma - ckg * (1 - cta)
    return cta


def next_theta(theta, kk, gamma, theta_eq):
    """theta of the iteration kk steps after a (re)start (accbpg/algorithms.py:142-145)."""
    return solve_theta(theta, gamma) if theta_eq and kk > 0 else gamma / (kk + gamma)


class _Run:
    """The full-length result arrays named in ``records`` (F[k - 1] at k = 0 is a zero of them), the last iteration
    that ran and the tuple cut to it."""

    def __init__(self, maxitrs):
        for name in self.records:
            setattr(self, name, np.zeros(maxitrs))
        self.k = -1

    def record(self, Fk, now):
        """F(x) = Fk of this iteration, known at time ``now``."""
        self.F[self.k] = Fk
        self.T[self.k] = now

    def result(self, x):
        return (x,) + tuple(getattr(self, name)[:self.k + 1] for name in self.records)


class _BPGRun(_Run):
    """One instance of BPG: L and its backtracking search, the records and the stop test."""
    records = ("F", "Ls", "T")

    def __init__(self, L, maxitrs, epsilon, linesearch, ls_ratio):
        super().__init__(maxitrs)
        self.L, self.epsilon, self.linesearch, self.ls_ratio = L, epsilon, linesearch, ls_ratio
        self.Ls = np.ones(maxitrs) * L

    def begin(self, k, Fk, now):
        """Iteration k, its F and T; L is divided before a search (:51)."""
        self.k = k
        self.record(Fk, now)
        if self.linesearch:
            self.L = self.L / self.ls_ratio

    def accepts(self, ft, fx, lin, dist):
        """The test of a trial with value ft, <g, trial - x> = lin and D(trial, x) = dist (:53); L is multiplied when
        it fails (:54)."""
        if not (ft > fx + lin + self.L * dist):
            return True
        self.L = self.L * self.ls_ratio
        return False

    def finish(self):
        """Records L_k; True when the stop test holds (:66)."""
        self.Ls[self.k] = self.L
        return self.k > 0 and abs(self.F[self.k] - self.F[self.k - 1]) < self.epsilon


class _Accelerated(_Run):
    """What ABPG and ABPG_gain share: theta and its restart, and the stop test on D(z+, z)."""

    def __init__(self, L, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule):
        super().__init__(maxitrs)
        self.L, self.gamma, self.epsilon, self.theta_eq = L, gamma, epsilon, theta_eq
        self.restart, self.restart_rule = restart, restart_rule
        self.theta, self.kk = 1.0, 0
        self.dzz = None             # D(z+, z) of the last step: the stop test reads it

    def needs_dot(self):
        """Whether ``finish`` reads <g, x+ - x>."""
        return self.restart and self.restart_rule == 'g' and self.k >= self.restart_from

    def finish(self, dot=None):
        """(restarted, stop): restarted -- the caller sets z = x+; stop -- D(z+, z) < epsilon."""
        k, F = self.k, self.F
        self.kk += 1
        restarted = False
        if self.restart and k >= self.restart_from:
            if (self.restart_rule == 'f' and F[k] > F[k - 1]) or (self.restart_rule == 'g' and dot > 0):
                self.theta, self.kk = 1.0, 0
                restarted = True
        return restarted, self.dzz < self.epsilon


class _ABPGRun(_Accelerated):
    """One instance of ABPG: theta, the restart state (:165-171), the records and the stop test (:174)."""
    records = ("F", "G", "T")
    restart_from = 1

    def begin(self, k):
        """Iteration k: advances theta and returns it."""
        self.k = k
        self.theta = next_theta(self.theta, self.kk, self.gamma, self.theta_eq)
        return self.theta

    def prox_coef(self):
        return self.theta ** (self.gamma - 1) * self.L                      # :149

    def divergences(self, dxy, dzz):
        """D(x+, y) and D(z+, z) of the step: records and returns the triangle-scaling gain (:155)."""
        self.dzz = dzz
        self.G[self.k] = dxy / dzz / self.theta ** self.gamma
        return self.G[self.k]


# what a trial of ABPG_gain's search came to
BREAK, ACCEPT, RETRY, NEEDS_VALUE = "break", "accept", "retry", "needs f(x)"


class _GainRun(_Accelerated):
    """One instance of ABPG_gain: the gain and its search, theta, the restart state (:403-409), the records and the
    stop test (:412).

    Quirks kept: the gain is cut by ls_dec before every search (:358); an inner break on D(z+,z) < epsilon records
    the previous Gdr (:379-382, NameError in the reference if that happens at k = 0 -- here it records 0.0); the
    restart test has no k > 0 guard, so rule 'f' at k = 0 compares with F[-1] (:403-406)."""
    records = ("F", "Gain", "Gdiv", "Gavg", "T")
    restart_from = 0

    def __init__(self, L, gamma, maxitrs, epsilon, G0, ls_inc, ls_dec, theta_eq, checkdiv, restart, restart_rule):
        super().__init__(L, gamma, maxitrs, epsilon, theta_eq, restart, restart_rule)
        self.ls_inc, self.ls_dec, self.checkdiv = ls_inc, ls_dec, checkdiv
        self.Gain = np.ones(maxitrs) * G0
        self.G, self.Gdr = G0, 0.0
        self.sumlogG = gamma * np.log(G0)                                   # :342
        self.lin = self.G_prev = self.theta_prev = None     # of the trial / the iteration under way
        self.failed = 0             # failed trials of this iteration ...
        self.retries_before = 0     # ... and of the one before: how far ahead a caller may start gradients

    def begin(self, k):
        """Iteration k: remembers the gain and theta it starts from and cuts the gain (:358)."""
        self.k = k
        self.G_prev, self.theta_prev = self.G, self.theta
        self.G = self.G / self.ls_dec
        self.retries_before, self.failed = self.failed, 0

    def theta_for(self, G):
        """theta of a trial with gain G (:362-367); for G * ls_inc, of the trial after a failure of the present one."""
        if self.kk == 0:
            return self.theta
        if self.theta_eq:
            return solve_theta(self.theta_prev, self.gamma, G / self.G_prev)
        alpha = G / self.G_prev
        return self.theta_prev * ((1 + alpha * (self.gamma - 1)) / (self.gamma * alpha + self.theta_prev))

    def trial(self):
        """Sets and returns theta of the trial at the present gain."""
        self.theta = self.theta_for(self.G)
        return self.theta

    def prox_coef(self):
        return self.theta ** (self.gamma - 1) * self.G * self.L             # :373

    def divergences(self, lin, dxy, dzz):
        """<g, x+ - y>, D(x+, y) and D(z+, z) of a trial.  BREAK: the search ends with Gdr left as it was (:379-380);
        NEEDS_VALUE: ``value`` decides; ACCEPT or RETRY: checkdiv decided (:385)."""
        self.lin, self.dzz = lin, dzz
        if dzz < self.epsilon:
            return BREAK
        self.Gdr = dxy / dzz / self.theta ** self.gamma                     # :382
        return self._decided(self.Gdr > self.G) if self.checkdiv else NEEDS_VALUE

    def value(self, fx, fy):
        """ACCEPT or RETRY by the values at x+ and y (:387)."""
        return self._decided(fx > fy + self.lin + self.theta ** self.gamma * self.G * self.L * self.dzz)

    def _decided(self, retry):
        if not retry:
            return ACCEPT
        self.G = self.G * self.ls_inc                                       # :390
        self.failed += 1
        return RETRY

    def finish(self, dot=None):
        """Records the gain, Gdr and the running average (:395-396), then the restart and the stop test."""
        k = self.k
        self.Gain[k] = self.G
        self.Gdiv[k] = self.Gdr
        self.sumlogG += np.log(self.G)
        self.Gavg[k] = np.exp(self.sumlogG / (self.gamma + k))
        return super().finish(dot)


class _ExpoRun(_Accelerated):
    """One instance of ABPG_expo (:183-292): the exponent and its lowering, theta, the restart state (:276-282), the
    records and the stop test (:285).

    Quirks kept: theta is that of the exponent the iteration starts from, for all of its trials (:238-241); a failed
    test at gamma == 1 is accepted (:262-265); a comparison with a NaN is False, which accepts; the restart test has no
    k > 0 guard, so rule 'f' at k = 0 compares with F[-1] (:276-279)."""
    records = ("F", "Gamma", "G", "T")
    restart_from = 0

    def __init__(self, L, gamma0, maxitrs, epsilon, delta, theta_eq, checkdiv, Gmargin, restart, restart_rule):
        super().__init__(L, gamma0, maxitrs, epsilon, theta_eq, restart, restart_rule)
        self.delta, self.checkdiv, self.Gmargin = delta, checkdiv, Gmargin
        self.Gamma = np.ones(maxitrs) * gamma0
        self.lin, self.Gdr = None, 0.0

    def begin(self, k):
        """Iteration k: advances theta with the exponent it starts from and returns it."""
        self.k = k
        self.theta = next_theta(self.theta, self.kk, self.gamma, self.theta_eq)     # :238-241
        return self.theta

    def prox_coef(self):
        return self.theta ** (self.gamma - 1) * self.L                      # :249

    def divergences(self, lin, dxy, dzz):
        """<g, x+ - y>, D(x+, y) and D(z+, z) of a trial.  NEEDS_VALUE: ``value`` decides; ACCEPT or RETRY: checkdiv
        decided (:258)."""
        self.lin, self.dzz = lin, dzz
        self.Gdr = dxy / dzz / self.theta ** self.gamma                     # :255
        if self.checkdiv:
            return self._decided(dxy > self.Gmargin * (self.theta ** self.gamma) * dzz)
        return NEEDS_VALUE

    def value(self, fx, fy):
        """ACCEPT or RETRY by the values at x+ and y (:260)."""
        return self._decided(fx > fy + self.lin + self.theta ** self.gamma * self.L * self.dzz)

    def _decided(self, failed):
        if failed and self.gamma > 1:                                       # :262-265
            self.gamma = max(self.gamma - self.delta, 1)
            return RETRY
        return ACCEPT

    def finish(self, dot=None):
        """Records Gdr and the exponent (:267-268), then the restart and the stop test."""
        self.G[self.k] = self.Gdr
        self.Gamma[self.k] = self.gamma
        return super().finish(dot)


class _ABDARun(_Accelerated):
    """One instance of ABDA (:423-514): theta, the running sum of the weights, the records and the stop test (:508)."""
    records = ("F", "G", "T")
    restart_from = 0            # (never read: ABDA does not restart)

    def __init__(self, L, gamma, maxitrs, epsilon, theta_eq):
        super().__init__(L, gamma, maxitrs, epsilon, theta_eq, False, 'g')
        self.csum = 0                                                       # the integer, as in the reference (:463)

    def begin(self, k):
        """Iteration k: advances theta and returns it."""
        self.k = k
        self.theta = next_theta(self.theta, self.kk, self.gamma, self.theta_eq)     # :472-475
        return self.theta

    def weight(self):
        """(theta^(1-gamma), the sum of the weights with it, L over that sum): gavg += wgt * g (:483), csum += wgt
        (:484), z = prox_map(gavg / csum, L / csum) (:485)."""
        wgt = self.theta ** (1 - self.gamma)
        self.csum = self.csum + wgt
        return wgt, self.csum, self.L / self.csum

    def divergences(self, dxy, dzz):
        """D(x+, y) and D(z+, z) of the step: records and returns the triangle-scaling gain (:491)."""
        self.dzz = dzz
        self.G[self.k] = dxy / dzz / self.theta ** self.gamma
        return self.G[self.k]


# ---------------------------------------------------------------------------------------------------------------
# The (L0, L1) Frank-Wolfe family (accbpg/algorithms_fw.py:78-207, :250-349, :352-453).  A run object takes the
# scalars of an iteration -- f(x), ||g||, <g, d>, and D(s, x) or ||d|| -- and decides: the division of L0 and L1 in
# front of a search, the step, the acceptance test, which constant grows when it fails, their caps, the records and the
# stop test.  The traces are lists, as in the reference: LOG_STEPS gains an entry per trial.  ``lhs`` and ``rhs`` are
# the two sides of the last acceptance test.  Arguments are taken as NumPy scalars and math / NumPy routines are the
# reference's, so that the bits are.
# ---------------------------------------------------------------------------------------------------------------
_L0L1_BAND = 1e-8           # the slopes in (0, band] counted as 0, and the stand-in for a vanishing divergence


class _L0L1Run:
    lo_message = "Initial L0 and L1 must be positive"
    slope_message = "grad_d_prod must be non-positive (we minimize)"

    def __init__(self, L0, L1, epsilon, linesearch, ls_ratio):
        for bad, message in ((ls_ratio < 1, "ls_ratio must be >= 1"),
                             (self.bad_start(L0, L1), self.lo_message),
                             (epsilon <= 0, "epsilon must be positive")):
            if bad:
                raise ValueError(message)
        self.L0, self.L1, self.epsilon, self.linesearch, self.ls_ratio = L0, L1, epsilon, linesearch, ls_ratio
        self.F, self.Ls, self.T = [], [], []
        self.k, self.toggle = -1, 0
        self.lhs = self.rhs = None

    @staticmethod
    def bad_start(L0, L1):
        return L0 <= 0 or L1 <= 0

    def begin(self, k, fx, Fk, now):
        """Iteration k with f(x) = fx and F(x) = Fk known at time ``now``."""
        self.k, self.fx = k, fx
        self.F.append(Fk)
        self.T.append(now)

    def banded(self, slope):
        """<g, d> with the band (0, 1e-8] set to the integer 0; a larger one is the oracle's fault."""
        if 0 < slope <= _L0L1_BAND:
            slope = 0
        if slope > 0:
            raise ValueError(self.slope_message)
        return slope

    def decide(self, ft, rhs):
        self.lhs, self.rhs = ft, rhs
        return ft <= rhs

    def finish(self):
        """Records a_k; True when the stop test holds."""
        self.Ls.append(self.a_k)
        return self.k > 0 and bool(abs(self.F[self.k] - self.F[self.k - 1]) < self.epsilon)

    def result(self, x):
        return x, np.array(self.F), np.array(self.Ls), np.array(self.T)


class _ShortestStepRun(_L0L1Run):
    """One instance of FW_alg_L0_L1_shortest_step (:78-207).

    Quirks kept: ``L0 /= ls_ratio + L0 / a_k`` divides by the whole sum (:175-176) and ``L0 *= ls_ratio - L0 / a_k``
    multiplies by the whole difference (:192, :195); the toggle that picks the constant to grow lives across
    iterations (:153); a divergence of exactly 0 becomes 1e-8 (:162-163); zero constants are allowed and the message
    for negative ones says "positive" (:138-139)."""
    lo_message = "Initial L must be positive"
    slope_message = "⟨∇f(x), d⟩ must be nonpositive (LMO issue)."

    def __init__(self, L0, L1, gamma, epsilon, linesearch, ls_ratio):
        super().__init__(L0, L1, epsilon, linesearch, ls_ratio)
        self.gamma = gamma

    @staticmethod
    def bad_start(L0, L1):
        return L0 < 0 or L1 < 0

    def direction(self, gnorm, slope, div):
        """||g||, <g, d> and D(s, x) of the iteration; divides L0 and L1 in front of a search (:174-176)."""
        if div == 0:
            div = _L0L1_BAND
        self.gnorm, self.div, self.slope = gnorm, div, self.banded(slope)
        a_k = self.L0 + self.L1 * gnorm
        if self.linesearch:
            self.L0 /= self.ls_ratio + self.L0 / a_k
            self.L1 /= self.ls_ratio + (self.L1 * gnorm) / a_k
        return True

    def step(self):
        """The step of a trial with the current constants (:179-182)."""
        self.a_k = self.L0 + self.L1 * self.gnorm
        self.alpha = min((-self.slope / (self.a_k * self.div * np.e)) ** (1 / (self.gamma - 1)), 1)
        return self.alpha

    def accepts(self, ft):
        """The test of the trial's value ft (:188); the constant the toggle names grows when it fails (:191-196)."""
        a, a_k = self.alpha, self.a_k
        if self.decide(ft, self.fx + a * self.slope + a ** self.gamma * (a_k / 2) * np.e * self.div):
            return True
        if self.toggle == 0:
            self.L0 *= self.ls_ratio - self.L0 / a_k
            self.toggle = 1
        else:
            self.L1 *= self.ls_ratio - (self.L1 * self.gnorm) / a_k
            self.toggle = 0
        return False


class _LogStepRun(_L0L1Run):
    """What FW_l0l1_log_and_linear_step and FW_l0l1_log_only share: LOG_STEPS, which starts with a 0 and gains an entry
    per trial (:304-305, :314, :317), the caps, which are tested for truth so that a cap of 0 is no cap (:336-337), the
    model exp(z) - 1 - z of the acceptance test with 0.5 z^2 in its place from z = 50 on (:326-332), and the ending at
    d = 0: the reference divides by ||d|| = 0 there and goes on with NaN; ``direction`` returns False and the run ends
    with what has been recorded -- F and T have that iteration's entry, Ls has not."""

    def __init__(self, L0, L1, ls_ratio, epsilon, L0_max, L1_max, linesearch):
        super().__init__(L0, L1, epsilon, linesearch, ls_ratio)
        self.L0_max, self.L1_max = L0_max, L1_max
        self.LOG_STEPS = []

    def direction(self, gnorm, slope, dnorm):
        """||g||, <g, d> and ||d|| of the iteration; False at d = 0.  Divides L0 and L1 in front of a search."""
        self.gnorm, self.dnorm, self.slope = gnorm, dnorm, self.banded(slope)
        if self.k == 0:
            self.LOG_STEPS.append(0)
        if dnorm == 0:
            return False
        if self.linesearch:
            self.L0 /= self.ls_ratio
            self.L1 /= self.ls_ratio
        self.floor_L1()
        return True

    def floor_L1(self):
        pass

    def grown(self, L, cap):
        return min(L * self.ls_ratio, cap) if cap else L * self.ls_ratio

    def accepts(self, ft):
        """The test of the trial's value ft (:326-333); ``grow`` when it fails."""
        z = self.L1 * self.alpha * self.dnorm
        if z < 50:
            exp_term = np.expm1(z) - z
        else:
            exp_term = 0.5 * z**2
        if self.decide(ft, self.fx + self.alpha * self.slope + (self.a_k / self.L1**2) * exp_term):
            return True
        self.grow()
        self.a_k = self.L0 + self.L1 * self.gnorm
        return False

    def result(self, x):
        return x, np.array(self.F), np.array(self.Ls), np.array(self.LOG_STEPS), np.array(self.T)


class _LogLinearRun(_LogStepRun):
    """One instance of FW_l0l1_log_and_linear_step (:250-349): the logarithmic step when L1 ||d|| >= log 2 (np.log),
    the linear one below; both constants grow on a failed test."""

    def step(self):
        assert self.L0 >= 0 and self.L1 >= 0, "Smoothness parameters must stay positive"
        L1, d_norm, slope = self.L1, self.dnorm, self.slope
        self.a_k = a_k = self.L0 + L1 * self.gnorm
        if L1 * d_norm >= np.log(2):
            self.alpha = (1 / (L1 * d_norm)) * np.log(1 - (L1 * slope) / (a_k * d_norm))
            self.LOG_STEPS.append(self.LOG_STEPS[-1] + 1)
        else:
            self.alpha = L1 * (-slope) / (a_k * d_norm)
            self.LOG_STEPS.append(self.LOG_STEPS[-1])
        return self.alpha

    def grow(self):
        self.L0 = self.grown(self.L0, self.L0_max)
        self.L1 = self.grown(self.L1, self.L1_max)


class _LogOnlyRun(_LogStepRun):
    """One instance of FW_l0l1_log_only (:352-453): L1 is lifted to log 2 / ||d|| after the division (:402), so every
    step is the logarithmic one (math.log); a failed test grows L0 and L1 in turn, the toggle living across
    iterations (:378)."""

    def floor_L1(self):
        self.L1 = max(math.log(2) / self.dnorm, self.L1)

    def step(self):
        assert self.L0 >= 0 and self.L1 >= 0, "Smoothness parameters must stay positive"
        L1, d_norm, slope = self.L1, self.dnorm, self.slope
        self.a_k = a_k = self.L0 + L1 * self.gnorm
        z = L1 * d_norm
        if z >= math.log(2) - 1e-5:
            self.alpha = (1 / (L1 * d_norm)) * math.log(1 - (L1 * slope) / (a_k * d_norm))
            self.LOG_STEPS.append(self.LOG_STEPS[-1] + 1)
        else:
            assert False, "No use for the second step!"
        return self.alpha

    def grow(self):
        if self.toggle == 0:
            self.L0 = self.grown(self.L0, self.L0_max)
            self.toggle = 1
        else:
            self.L1 = self.grown(self.L1, self.L1_max)
            self.toggle = 0
