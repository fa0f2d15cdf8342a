"""The host decisions of ABPG_expo and ABDA live in accbpg_and_fw_amd/solver_runs.py (_ExpoRun, _ABDARun), one copy for
the sequential solvers and the lock-step batches.  Driven here without a device, as tests/test_solver_runs_cpu.py drives
the other runs: (a) NumPy loops that take every decision from the run objects and do the vector work with the oracle's
objective and kernel reproduce oracle.np_oracle's solvers exactly; (b) records that need particular numbers (a failing
test at gamma = 1, the clamp, NaN in a comparison, rule 'f' at k = 0, the first weight sum) are scripted by hand.
No GPU, no torch, no library load."""
import importlib.util
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import np_oracle as O  # noqa: E402

MODULE = os.path.join(ROOT, "accbpg_and_fw_amd", "solver_runs.py")
_spec = importlib.util.spec_from_file_location("solver_runs_expo_abda_under_test", MODULE)   # (not the package: no torch)
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

NAN = float("nan")
M, N, ITERS = 8, 40, 60


@pytest.fixture(scope="module")
def problem():
    V = np.random.RandomState(1).randn(M, N)
    V.setflags(write=False)
    return O.DOptOracle(V), O.BurgSimplexOracle(), np.ones(N) / N


# ---- (a) NumPy drivers: the vector work of the oracle, every decision from the run objects -------------------------
def drive_expo(f, h, L, x0, gamma0, maxitrs, epsilon=1e-14, delta=0.2, theta_eq=True, checkdiv=False, Gmargin=10,
               restart=False, restart_rule='g', trials=None):
    run = R._ExpoRun(L, gamma0, maxitrs, epsilon, delta, theta_eq, checkdiv, Gmargin, restart, restart_rule)
    x, z = np.copy(x0), np.copy(x0)
    for k in range(maxitrs):
        Fk = f(x) + h.extra_Psi(x)
        z_prev, x_prev = z, x
        theta = run.begin(k)
        run.record(Fk, 0.0)
        y = (1 - theta) * x_prev + theta * z_prev
        fy, g = f.func_grad(y)
        count = 0
        while True:
            assert run.theta == theta                           # fixed for all trials of the iteration
            z = h.div_prox_map(z_prev, g, run.prox_coef())
            x = (1 - theta) * x_prev + theta * z
            verdict = run.divergences(np.dot(g, x - y), h.divergence(x, y), h.divergence(z, z_prev))
            if verdict == R.NEEDS_VALUE:
                assert not checkdiv
                verdict = run.value(f(x), fy)
            count += 1
            if verdict != R.RETRY:
                assert verdict == R.ACCEPT
                break
        if trials is not None:
            trials.append(count)
        restarted, stop = run.finish(np.dot(g, x - x_prev) if run.needs_dot() else None)
        if restarted:
            z = x
        if stop:
            break
    return run.result(x)


def drive_abda(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, theta_eq=True):
    run = R._ABDARun(L, gamma, maxitrs, epsilon, theta_eq)
    x, z = np.copy(x0), np.copy(x0)
    gavg = np.zeros(x.size)
    for k in range(maxitrs):
        Fk = f(x) + h.extra_Psi(x)
        z_prev, x_prev = z, x
        theta = run.begin(k)
        run.record(Fk, 0.0)
        y = (1 - theta) * x_prev + theta * z_prev
        g = f.gradient(y)
        wgt, csum, Lc = run.weight()
        gavg = gavg + wgt * g
        z = h.prox_map(gavg / csum, Lc)
        x = (1 - theta) * x_prev + theta * z
        run.divergences(h.divergence(x, y), h.divergence(z, z_prev))
        restarted, stop = run.finish()
        assert not restarted
        if stop:
            break
    return run.result(x)


def same(got, want, records):
    """x and every record except T (the last): equal to the bit, the records cut to one length."""
    assert len(got) == len(want) == records + 2
    for a, b in zip(got[:-1], want[:-1]):
        np.testing.assert_array_equal(a, b)
    assert all(len(a) == len(want[1]) for a in got[1:])


EXPO_OPTS = [dict(gamma0=3, theta_eq=True),
             dict(gamma0=3, theta_eq=False, delta=0.5, restart=True),
             dict(gamma0=2.5, theta_eq=False, checkdiv=True, Gmargin=1, restart=True, restart_rule='f')]


@pytest.mark.parametrize("opts", EXPO_OPTS)
def test_expo_decisions_reproduce_the_oracle_solver(problem, opts):
    f, h, x0 = problem
    opts = dict(opts)
    gamma0 = opts.pop("gamma0")
    trials = []
    got = drive_expo(f, h, 1.0, x0, gamma0, ITERS, trials=trials, **opts)
    want = O.ABPG_expo(f, h, 1.0, x0, gamma0, ITERS, **opts)
    same(got, want, 3)
    assert len(got[1]) == ITERS
    Gamma = got[2]
    assert Gamma[-1] < gamma0 and np.all(np.diff(Gamma) <= 0)   # the exponent did come down, and never goes up
    assert max(trials) >= 2 and trials.count(1) > 0             # iterations that retried and iterations that did not
    assert sum(trials) - len(trials) >= len(set(Gamma)) - 1     # every lowering was a retry


@pytest.mark.parametrize("theta_eq", [True, False])
def test_abda_decisions_reproduce_the_oracle_solver(problem, theta_eq):
    f, h, x0 = problem
    got = drive_abda(f, h, 1.0, x0, 2, ITERS, theta_eq=theta_eq)
    same(got, O.ABDA(f, h, 1.0, x0, 2, ITERS, theta_eq=theta_eq), 2)
    assert len(got[1]) == ITERS


@pytest.mark.parametrize("epsilon", [0.1, 0.03])
def test_stop_tests_and_cut_reproduce_the_oracle_solver(problem, epsilon):
    f, h, x0 = problem
    for got, want, records in [
            (drive_expo(f, h, 1.0, x0, 3, ITERS, epsilon), O.ABPG_expo(f, h, 1.0, x0, 3, ITERS, epsilon), 3),
            (drive_abda(f, h, 1.0, x0, 2, ITERS, epsilon), O.ABDA(f, h, 1.0, x0, 2, ITERS, epsilon), 2)]:
        same(got, want, records)
        assert len(got[1]) == len(want[1])


# ---- (b) scripted records --------------------------------------------------------------------------------------------
def test_expo_scripted_lowering_clamp_and_acceptance_at_one():
    L, gamma0, delta = 2.0, 1.75, 0.5
    run = R._ExpoRun(L, gamma0, 4, 0.01, delta, False, False, 10, False, 'g')
    assert run.records == ("F", "Gamma", "G", "T") and run.restart_from == 0
    np.testing.assert_array_equal(run.Gamma, np.full(4, gamma0))
    assert run.begin(0) == gamma0 / (0 + gamma0) == 1.0
    run.record(9.0, 0.5)
    assert run.prox_coef() == 1.0 ** (gamma0 - 1) * L
    assert run.divergences(0.25, 0.03, 0.5) == R.NEEDS_VALUE and run.Gdr == 0.03 / 0.5 / 1.0 ** gamma0
    bound = 1.0 + 0.25 + 1.0 ** gamma0 * L * 0.5                # fy + lin + theta^gamma L dzz = 2.25
    assert run.value(bound, 1.0) == R.ACCEPT and run.gamma == gamma0     # equality accepts
    assert run.value(np.nextafter(bound, 9.0), 1.0) == R.RETRY and run.gamma == 1.25     # 1.75 - 0.5
    assert run.theta == 1.0                                     # theta stays that of the iteration
    assert run.value(3.0, 1.0) == R.RETRY and run.gamma == 1    # delta = 0.5 > gamma - 1 = 0.25: clamps to 1
    assert run.prox_coef() == 1.0 ** (1 - 1) * L
    assert run.divergences(0.25, 0.06, 0.5) == R.NEEDS_VALUE
    assert run.value(3.0, 1.0) == R.ACCEPT and run.gamma == 1   # the test fails at gamma exactly 1: accepted
    assert run.needs_dot() is False
    assert run.finish() == (False, False)
    assert (run.G[0], run.Gamma[0]) == (0.06 / 0.5 / 1.0, 1)
    # k = 1: theta from the lowered exponent; NaN in the value test accepts; D(z+, z) < epsilon stops
    theta = run.begin(1)
    assert theta == 1 / (1 + 1)
    run.record(8.0, 1.5)
    assert run.divergences(0.25, 0.03, 0.005) == R.NEEDS_VALUE
    assert run.value(NAN, 1.0) == R.ACCEPT and run.value(1.0, NAN) == R.ACCEPT
    assert run.finish() == (False, True)
    x, F, Gamma, G, T = run.result("x")
    assert x == "x"
    np.testing.assert_array_equal(F, [9.0, 8.0])
    np.testing.assert_array_equal(Gamma, [1.0, 1.0])
    np.testing.assert_array_equal(G, [0.06 / 0.5 / 1.0, 0.03 / 0.005 / 0.5 ** 1])
    np.testing.assert_array_equal(T, [0.5, 1.5])
    assert R._ExpoRun(1.0, 3, 3, 0.01, 0.2, True, False, 10, False, 'g').result(None)[1].shape == (0,)


def test_expo_scripted_checkdiv_and_nan():
    gamma0, margin = 2, 3
    run = R._ExpoRun(1.0, gamma0, 4, 0.01, 0.25, True, True, margin, False, 'g')
    run.begin(0)
    run.record(9.0, 0.0)
    assert run.divergences(0.0, margin * 1.0 * 0.5, 0.5) == R.ACCEPT         # dxy = Gmargin theta^gamma dzz: > is false
    assert run.divergences(0.0, 1.75, 0.5) == R.RETRY and run.gamma == 1.75  # 1.75 > 3 * 1 * 0.5
    assert run.Gdr == 1.75 / 0.5 / 1.0 ** 2                                  # Gdr is that of the exponent tried
    assert run.divergences(0.0, NAN, 0.5) == R.ACCEPT and np.isnan(run.Gdr)  # nan > ... is false
    assert run.divergences(0.0, 1.75, NAN) == R.ACCEPT and run.gamma == 1.75
    run.finish()
    assert np.isnan(run.G[0]) and run.Gamma[0] == 1.75
    assert run.begin(1) == O.solve_theta(1.0, 1.75)             # theta_eq, kk > 0, the exponent the iteration starts from
    run.record(8.0, 0.0)
    theta = run.theta
    assert run.divergences(0.0, 1.0, 0.5) == R.RETRY and run.gamma == 1.5    # 1 > 3 theta^1.75 / 2 (theta about 0.64)
    assert run.theta == theta and run.prox_coef() == theta ** (1.5 - 1) * 1.0
    assert run.divergences(0.0, 0.0, 0.5) == R.ACCEPT
    assert run.Gdr == 0.0 / 0.5 / theta ** 1.5


def expo_step(run, k, Fk, dot=None):
    theta = run.begin(k)
    run.record(Fk, 0.0)
    assert run.divergences(0.0, 0.03, 0.5) == R.NEEDS_VALUE and run.value(0.0, 1.0) == R.ACCEPT
    needs = run.needs_dot()
    return (theta, needs) + run.finish(dot if needs else None)


def test_expo_restart_has_no_k0_guard():
    run = R._ExpoRun(1.0, 2, 5, 0.01, 0.2, False, False, 10, True, 'f')
    assert expo_step(run, 0, 5.0) == (1.0, False, True, False)  # F[0] = 5 > F[-1] = 0: restarts at k = 0
    assert (run.theta, run.kk) == (1.0, 0)
    assert expo_step(run, 1, 4.0) == (1.0, False, False, False)     # kk = 0 after the restart
    assert run.kk == 1
    theta, _, restarted, _ = expo_step(run, 2, 4.5)
    assert theta == 2 / (1 + 2) and restarted and (run.theta, run.kk) == (1.0, 0)       # F rose
    assert expo_step(run, 3, NAN)[2] is False                   # nan > F is false
    neg = R._ExpoRun(1.0, 2, 5, 0.01, 0.2, False, False, 10, True, 'f')
    assert expo_step(neg, 0, -5.0)[2] is False                  # -5 > F[-1] = 0 is false
    g = R._ExpoRun(1.0, 2, 5, 0.01, 0.2, False, False, 10, True, 'g')
    assert expo_step(g, 0, 5.0, dot=0.5) == (1.0, True, True, False)         # asked for and acted on at k = 0
    assert expo_step(g, 1, 4.0, dot=-0.5)[1:] == (True, False, False)
    assert expo_step(g, 2, 3.0, dot=NAN)[1:] == (True, False, False)
    off = R._ExpoRun(1.0, 2, 5, 0.01, 0.2, False, False, 10, False, 'f')
    assert expo_step(off, 0, 5.0)[1:] == (False, False, False)


def test_abda_scripted_weights_and_records():
    L, gamma = 3.0, 2
    run = R._ABDARun(L, gamma, 4, 0.01, False)
    assert run.records == ("F", "G", "T")
    assert run.csum == 0 and isinstance(run.csum, int)          # the integer 0, as in the reference
    assert run.begin(0) == 2 / (0 + 2)
    run.record(9.0, 0.5)
    wgt, csum, Lc = run.weight()
    assert wgt == 1.0 ** (1 - gamma) and csum == 0 + wgt and Lc == L / csum
    assert run.divergences(0.03, 0.5) == 0.03 / 0.5 / 1.0 ** gamma and run.G[0] == 0.03 / 0.5
    assert run.needs_dot() is False
    assert run.finish() == (False, False)
    theta = run.begin(1)
    assert theta == 2 / (1 + 2)
    run.record(8.0, 1.5)
    wgt2, csum2, Lc2 = run.weight()
    assert wgt2 == theta ** (1 - gamma) and csum2 == csum + wgt2 and Lc2 == L / csum2
    assert run.divergences(0.03, NAN) != run.G[1]               # nan recorded
    assert run.finish() == (False, False)                       # nan < epsilon is false
    run.begin(2)
    run.record(7.0, 2.5)
    run.weight()
    run.divergences(0.02, 0.005)
    assert run.finish() == (False, True)
    x, F, G, T = run.result("x")
    np.testing.assert_array_equal(F, [9.0, 8.0, 7.0])
    np.testing.assert_array_equal(T, [0.5, 1.5, 2.5])
    assert len(G) == 3 and np.isnan(G[1]) and G[2] == 0.02 / 0.005 / (2 / 4) ** gamma
    eq = R._ABDARun(1.0, 2, 3, 0.01, True)
    eq.begin(0)
    eq.divergences(0.03, 0.5)
    eq.finish()
    assert eq.begin(1) == O.solve_theta(1.0, 2)                 # theta_eq and kk > 0
