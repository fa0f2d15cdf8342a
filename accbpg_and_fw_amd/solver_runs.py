"""The host decisions of BPG / ABPG / ABPG_expo / ABPG_gain / ABDA (accbpg/algorithms.py:11-514), one copy for the single
solvers of ``algorithms.py`` and the lock-step batches of ``batched.py``, as ``_DivStepRun`` / ``_DescentRun`` are for the
Frank-Wolfe solvers.  A run object is one instance's scalars, result arrays and last iteration; it touches no device
and no vector -- the caller does that work and hands over the numbers -- so the CPU tests drive it with NumPy
(tests/test_solver_runs_cpu.py).  Every expression keeps the reference's operation order; the cited lines are its."""
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
