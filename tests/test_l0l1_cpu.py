"""CPU tests of the (L0, L1) Frank-Wolfe family: the run objects of accbpg_and_fw_amd/solver_runs.py against the goldens
of the real reference (tests/golden/l0l1.npz, tools/gen_golden_l0l1.py) and on scripted cases, one per quirk of the
reference that they keep; the public names and signatures; the instance generators and the LIBSVM loader."""
import inspect
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l0l1_numpy as LL  # noqa: E402
from conftest import golden  # noqa: E402

from accbpg_and_fw_amd import solver_runs as R  # noqa: E402

NEW_ENTRIES = ("accbpg_fw_direction", "accbpg_logistic_line_begin", "accbpg_logistic_line_value",
               "accbpg_logistic_line_accept", "accbpg_logistic_func_grad_carried")
NP_LMO = {"l2": LL.lmo_l2_ball, "linf": LL.lmo_linf_ball, "simplex": LL.lmo_simplex}


@pytest.fixture(scope="module")
def gold():
    return golden("l0l1")


@pytest.fixture(scope="module")
def problem(gold):
    A, y = LL.instance()
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["A_checksum"], rtol=1e-14)
    assert np.array_equal(y, gold["y"])
    return A, y


# -------------------------------------------------------------------------------------------------------- goldens
@pytest.mark.parametrize("domain", LL.DOMAINS)
@pytest.mark.parametrize("solver", LL.SOLVERS)
def test_run_objects_reproduce_the_reference(gold, problem, solver, domain):
    A, y = problem
    key = "%s_%s" % (solver, domain)
    f, tests = LL.StandIn(A, y), []
    run = LL.make_run(R, solver, LL.run_params(solver, domain, A))
    res = LL.drive(run, f, LL.SquaredL2Norm(), LL.start(domain, A.shape[1]), LL.ITERS, NP_LMO[domain](LL.RADIUS[domain]),
                   solver == "shortest", tests)
    x, F, Ls = res[:3]
    assert int(gold[key + "_prefix"]) == len(gold[key + "_F"]) == len(F) == LL.ITERS
    assert np.array_equal(Ls, gold[key + "_Ls"])
    assert f.values == int(gold[key + "_trials"]) == len(tests)
    if solver != "shortest":
        assert np.array_equal(res[3], gold[key + "_LOG"]) and len(res[3]) == f.values + 1 and res[3][0] == 0
        assert len(res) == 5
    Fr = gold[key + "_F"]
    assert np.all(np.abs(F - Fr) <= 1e-9 * (1 + np.abs(Fr)))
    assert np.max(np.abs(x - gold[key + "_x"])) <= float(gold[key + "_xspread"]) + 1e-12
    assert min(abs(a - b) for a, b in tests) == float(gold[key + "_min_margin"])
    assert sum(1 for a, b in tests if not a <= b) == int(gold[key + "_fails"])


def test_goldens_show_what_the_generator_promises(gold, problem):
    A, _ = problem
    keys = ["%s_%s" % (s, d) for s in LL.SOLVERS for d in LL.DOMAINS]
    assert any(int(gold[k + "_fails"]) >= 2 for k in keys if not k.startswith("loglin"))       # either toggle
    steps = np.concatenate([np.diff(gold["loglin_%s_LOG" % d]) for d in LL.DOMAINS])
    assert np.any(steps == 1) and np.any(steps == 0)                                         # both kinds of step
    for k in keys:
        carried = (LL.REFRESH - 1) * LL.value_step_bound(A, k.split("_")[1]) + 6 * LL.LN.U * float(np.max(gold[k + "_F"]))
        assert float(gold[k + "_min_margin"]) > 1000 * carried, k


# ------------------------------------------------------------------------------------------------ scripted quirks
def test_shortest_step_divides_by_the_whole_sum_and_grows_in_turn():
    run = R._ShortestStepRun(1.0, 2.0, 2.0, 1e-14, True, 2)
    run.begin(0, np.float64(5.0), np.float64(5.0), 0.0)
    g, slope, div = np.float64(3.0), np.float64(-0.5), np.float64(0.25)
    assert run.direction(g, slope, div)
    assert run.L0 == 1.0 / (2 + 1.0 / 7.0) and run.L1 == 2.0 / (2 + (2.0 * 3.0) / 7.0)      # L0 /= ls_ratio + L0 / a_k
    L0, L1 = run.L0, run.L1
    a_k = L0 + L1 * g
    alpha = run.step()
    assert alpha == min((0.5 / (a_k * div * np.e)) ** (1 / (2.0 - 1)), 1) and run.a_k == a_k
    rhs = 5.0 + alpha * slope + alpha ** 2.0 * (a_k / 2) * np.e * div
    assert run.accepts(np.nextafter(rhs, np.inf)) is False and run.rhs == rhs
    assert run.L0 == L0 * (2 - L0 / a_k) and run.L1 == L1 and run.toggle == 1                # L0 *= ls_ratio - L0 / a_k
    L0 = run.L0
    a_k = L0 + L1 * g
    alpha = run.step()
    assert run.accepts(np.float64(1e9)) is False
    assert run.L1 == L1 * (2 - (L1 * g) / a_k) and run.L0 == L0 and run.toggle == 0
    run.step()
    assert run.accepts(run.rhs) is True                                                    # <= accepts equality
    assert run.finish() is False and run.Ls == [run.a_k]
    # the toggle lives across iterations
    run.begin(1, np.float64(5.0), np.float64(5.0), 0.0)
    run.direction(g, slope, div)
    L1 = run.L1
    run.step()
    run.accepts(np.float64(1e9))
    assert run.toggle == 1 and run.L1 == L1
    run.step()
    assert run.accepts(np.float64(-1e9)) and run.finish() is True                          # |F[1] - F[0]| = 0 < epsilon
    x, F, Ls, T = run.result("x")
    assert x == "x" and len(F) == len(Ls) == len(T) == 2


def test_shortest_step_band_floor_and_messages():
    run = R._ShortestStepRun(0.0, 1.0, 2.0, 1e-14, False, 2)                                 # zero constants are allowed
    run.begin(0, np.float64(1.0), np.float64(1.0), 0.0)
    run.direction(np.float64(2.0), np.float64(1e-8), np.float64(0.0))
    assert run.slope == 0 and isinstance(run.slope, int) and run.div == 1e-8               # the band and the floor
    assert (run.L0, run.L1) == (0.0, 1.0)                                                  # no search: no division
    assert run.step() == 0
    run.direction(np.float64(2.0), np.float64(-3.0), np.float64(1e-30))
    assert run.div == 1e-30 and run.step() == 1                                            # only an exact 0 is replaced
    with pytest.raises(ValueError, match=re.escape("⟨∇f(x), d⟩ must be nonpositive (LMO issue).")):
        run.direction(np.float64(2.0), np.float64(1.0000001e-8), np.float64(1.0))
    for args, text in (((1.0, 1.0, 2.0, 1e-14, True, 0.5), "ls_ratio must be >= 1"),
                       ((-1.0, 1.0, 2.0, 1e-14, True, 2), "Initial L must be positive"),
                       ((1.0, -1.0, 2.0, 1e-14, True, 2), "Initial L must be positive"),
                       ((1.0, 1.0, 2.0, 0.0, True, 2), "epsilon must be positive")):
        with pytest.raises(ValueError, match=re.escape(text)):
            R._ShortestStepRun(*args)
    for cls in (R._LogLinearRun, R._LogOnlyRun):
        for args, text in (((1.0, 1.0, 0.5, 1e-14, None, None, True), "ls_ratio must be >= 1"),
                           ((0.0, 1.0, 2.0, 1e-14, None, None, True), "Initial L0 and L1 must be positive"),
                           ((1.0, 0.0, 2.0, 1e-14, None, None, True), "Initial L0 and L1 must be positive"),
                           ((1.0, 1.0, 2.0, -1.0, None, None, True), "epsilon must be positive")):
            with pytest.raises(ValueError, match=re.escape(text)):
                cls(*args)
        run = cls(1.0, 1.0, 2.0, 1e-14, None, None, True)
        run.begin(0, np.float64(1.0), np.float64(1.0), 0.0)
        with pytest.raises(ValueError, match=re.escape("grad_d_prod must be non-positive (we minimize)")):
            run.direction(np.float64(1.0), np.float64(0.5), np.float64(1.0))


def test_log_and_linear_step_formulas_log_steps_and_caps():
    run = R._LogLinearRun(4.0, 8.0, 2.0, 1e-14, 0, 5.0, True)                                # L0_max = 0: no cap at all
    run.begin(0, np.float64(2.0), np.float64(2.0), 0.0)
    g, slope, dn = np.float64(3.0), np.float64(-0.7), np.float64(0.5)
    assert run.direction(g, slope, dn) and (run.L0, run.L1) == (2.0, 4.0) and run.LOG_STEPS == [0]
    a_k = 2.0 + 4.0 * g
    a = run.step()                                                                         # L1 ||d|| = 2 >= log 2
    assert a == (1 / (4.0 * dn)) * np.log(1 - (4.0 * slope) / (a_k * dn)) and run.LOG_STEPS == [0, 1]
    z = 4.0 * a * dn
    rhs = 2.0 + a * slope + (a_k / 4.0 ** 2) * (np.expm1(z) - z)
    assert run.accepts(np.nextafter(rhs, np.inf)) is False and run.rhs == rhs
    assert (run.L0, run.L1) == (4.0, 5.0) and run.a_k == 4.0 + 5.0 * g                     # both grow; L1 meets its cap
    run.step()
    assert run.LOG_STEPS == [0, 1, 2]                                                      # an entry per trial
    run.accepts(np.float64(1e9))
    assert (run.L0, run.L1) == (8.0, 5.0)                                                  # 0 is no cap, 5 is
    run.step()
    assert run.accepts(np.float64(-1.0)) and run.finish() is False and run.Ls == [8.0 + 5.0 * g]
    # the linear step below log 2, and no k = 0 entry later on
    run.begin(1, np.float64(1.0), np.float64(1.0), 0.0)
    dn = np.float64(0.1)
    run.direction(g, slope, dn)
    assert (run.L0, run.L1) == (4.0, 2.5) and run.LOG_STEPS == [0, 1, 2, 3]
    a = run.step()
    assert a == 2.5 * 0.7 / ((4.0 + 2.5 * g) * dn) and run.LOG_STEPS == [0, 1, 2, 3, 3]
    # z >= 50: the quadratic model in the place of expm1(z) - z
    run.alpha = np.float64(250.0)
    z = 2.5 * run.alpha * dn
    assert z >= 50
    run.accepts(np.float64(0.0))
    assert run.rhs == 1.0 + run.alpha * slope + (run.a_k / 2.5 ** 2) * (0.5 * z ** 2)
    run.alpha = np.float64(199.0)
    z = 2.5 * run.alpha * dn
    assert z < 50
    run.accepts(np.float64(0.0))
    assert run.rhs == 1.0 + run.alpha * slope + (run.a_k / 2.5 ** 2) * (np.expm1(z) - z)
    x, F, Ls, LOG, T = run.result(None)
    assert LOG.tolist() == [0, 1, 2, 3, 3] and len(F) == 2 and len(Ls) == 1
    # without a search one trial per iteration, the constants untouched
    run = R._LogLinearRun(4.0, 8.0, 2.0, 1e-14, None, None, False)
    run.begin(0, np.float64(2.0), np.float64(2.0), 0.0)
    run.direction(g, slope, np.float64(0.5))
    run.step()
    assert (run.L0, run.L1) == (4.0, 8.0) and run.LOG_STEPS == [0, 1] and run.finish() is False


def test_log_only_lifts_L1_and_grows_in_turn():
    run = R._LogOnlyRun(4.0, 1.0, 2.0, 1e-14, 6.0, None, True)
    run.begin(0, np.float64(2.0), np.float64(2.0), 0.0)
    g, slope, dn = np.float64(3.0), np.float64(-0.7), np.float64(0.5)
    run.direction(g, slope, dn)
    assert run.L0 == 2.0 and run.L1 == math.log(2) / dn                                    # max(log 2 / ||d||, L1 / 2)
    L1 = run.L1
    a = run.step()
    assert a == (1 / (L1 * dn)) * math.log(1 - (L1 * slope) / ((2.0 + L1 * g) * dn)) and run.LOG_STEPS == [0, 1]
    run.accepts(np.float64(1e9))
    assert (run.L0, run.L1, run.toggle) == (4.0, L1, 1)
    run.step()
    run.accepts(np.float64(1e9))
    assert (run.L0, run.L1, run.toggle) == (4.0, 2 * L1, 0)
    run.step()
    run.accepts(np.float64(1e9))
    assert (run.L0, run.L1, run.toggle) == (6.0, 2 * L1, 1)                                # L0 meets its cap
    run.step()
    assert run.accepts(np.float64(-1.0)) and run.LOG_STEPS == [0, 1, 2, 3, 4]
    run.finish()
    run.begin(1, np.float64(2.0), np.float64(2.0), 0.0)
    run.direction(g, slope, np.float64(100.0))
    assert run.L1 == L1 and run.toggle == 1                                                # L1 / 2 stays above the floor
    run.L1 = np.float64(1e-3)
    with pytest.raises(AssertionError, match="No use for the second step!"):
        run.step()
    run.L1 = np.float64(-1.0)
    with pytest.raises(AssertionError, match="Smoothness parameters must stay positive"):
        run.step()


@pytest.mark.parametrize("solver", ["loglin", "logonly"])
def test_log_runs_end_at_d_zero(solver):
    """an oracle that returns x itself: the reference would divide by ||d|| = 0; the run ends with what it has"""
    A, y = LL.instance(shape=(20, 6))
    run = LL.make_run(R, solver, dict(L0=1.0, L1=1.0, ls_ratio=2.0))
    calls = []

    def lmo(g):
        calls.append(1)
        return LL.lmo_l2_ball(1.0)(g) if len(calls) < 3 else np.copy(x_now[0])

    class Watch(LL.StandIn):
        def func_grad(self, x, flag=2):
            if flag == 2:
                x_now[0] = x
            return super().func_grad(x, flag)

    x_now = [None]
    with np.errstate(all="raise"):
        x, F, Ls, LOG, T = LL.drive(run, Watch(A, y), LL.SquaredL2Norm(), np.zeros(6), 10, lmo, False)
    assert len(F) == len(T) == 3 and len(Ls) == 2 and np.all(np.isfinite(F)) and np.array_equal(x, x_now[0])
    assert LOG[0] == 0 and len(LOG) >= 3
    run = LL.make_run(R, solver, dict(L0=1.0, L1=1.0, ls_ratio=2.0))
    x, F, Ls, LOG, T = LL.drive(run, LL.StandIn(A, y), LL.SquaredL2Norm(), np.ones(6), 10, lambda g: np.ones(6), False)
    assert len(F) == 1 and len(Ls) == 0 and LOG.tolist() == [0] and (run.L0, run.L1) == (1.0, 1.0)


# ------------------------------------------------------------------------------------------------ names and the ABI
def test_abi_and_python_names():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.accbpg_abi_version() == 3
    import accbpg_and_fw_amd as acc
    ours = ["fused", "carry", "refresh"]
    for name, prefix, defaults in (
            ("FW_alg_L0_L1_shortest_step",
             ["f", "h", "L0", "L1", "x0", "maxitrs", "gamma", "lmo", "epsilon", "linesearch", "ls_ratio", "verbose",
              "verbskip"], dict(epsilon=1e-14, linesearch=True, ls_ratio=2, verbose=True, verbskip=1)),
            ("FW_l0l1_log_and_linear_step",
             ["f", "h", "L0", "L1", "x0", "maxitrs", "lmo", "ls_ratio", "epsilon", "L0_max", "L1_max", "linesearch",
              "verbose", "verbskip"],
             dict(epsilon=1e-14, L0_max=None, L1_max=None, linesearch=True, verbose=True, verbskip=50)),
            ("FW_l0l1_log_only",
             ["f", "h", "L0", "L1", "x0", "maxitrs", "lmo", "ls_ratio", "epsilon", "L0_max", "L1_max", "linesearch",
              "verbose", "verbskip"],
             dict(epsilon=1e-14, L0_max=None, L1_max=None, linesearch=True, verbose=True, verbskip=50))):
        for fn in (name, name + "_steps"):
            assert fn in acc.__all__ and hasattr(acc, fn)
            sig = inspect.signature(getattr(acc, fn)).parameters
            assert list(sig) == prefix + ours
            assert {k: sig[k].default for k in defaults} == defaults
            assert all(sig[k].default is inspect.Parameter.empty for k in prefix if k not in defaults)
            assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ours)
            assert [sig[k].default for k in ours] == [True, False, 64]
    assert inspect.isgeneratorfunction(acc.FW_l0l1_log_only_steps)
    for name in ("line_begin", "line_value", "line_accept", "func_grad_carried"):
        assert hasattr(acc.LogisticRegression, name)
    for name in ("fw_direction", "toeplitz_matrix", "hard_FW_log_reg_jax", "L0L1_FW_log_reg", "load_a9a_data",
                 "L0L1_FW_log_reg_a9a"):
        assert name in acc.__all__ and hasattr(acc, name)
    sig = inspect.signature(acc.hard_FW_log_reg_jax).parameters
    assert list(sig) == ["key", "n_samples", "n_features", "radius", "domain", "k_sparse", "rho", "col_scale", "flip_y",
                         "margin", "class_bias", "x0_mode", "noise"]
    assert [sig[k].default for k in list(sig)[3:]] == [1.0, "l1", 5, 0.95, 10.0, 0.0, 0.5, 0.0, "center", 0.01]
    sig = inspect.signature(acc.L0L1_FW_log_reg).parameters
    assert list(sig) == ["key", "n_samples", "n_features", "ball_constrnt_radius", "solution_spread_radius_btm",
                         "solution_spread_radius_up", "noise", "rho"]
    assert [sig[k].default for k in list(sig)[4:]] == [0.91, 0.96, 0.0, 0.98]
    assert list(inspect.signature(acc.load_a9a_data).parameters) == ["path", "bias"]
    assert list(inspect.signature(acc.L0L1_FW_log_reg_a9a).parameters) == ["ball_constrnt_radius", "path"]
    # the oracles say what they are and stay the callables they were
    for lmo, kind in ((acc.lmo_l2_ball(2.0, 0.5), 0), (acc.lmo_linf_ball(2.0), 1), (acc.lmo_simplex(2.0), 2)):
        assert callable(lmo) and (lmo.kind, lmo.radius) == (kind, 2.0)
    assert acc.lmo_simplex().radius == 1 and acc.lmo_simplex().center is None
    assert acc.lmo_l2_ball(1.0, 0.5).center.center == 0.5 and acc.lmo_linf_ball(1.0).center.center is None


# --------------------------------------------------------------------------------------------------- the generators
class Recorded:
    """in the place of the device objective: keeps what it was built from"""

    def __init__(self, X, y):
        self.X, self.y = X, y


@pytest.fixture()
def apps(monkeypatch):
    from accbpg_and_fw_amd import applications
    monkeypatch.setattr(applications, "LogisticRegression", Recorded)
    return applications


def test_toeplitz_matrix(apps):
    T = apps.toeplitz_matrix(5, 0.5)
    assert T.shape == (5, 5) and np.array_equal(T, T.T) and np.all(np.diag(T) == 1.0) and T[0, 4] == 0.5 ** 4
    assert np.array_equal(T, LL.toeplitz(5, 0.5))


@pytest.mark.parametrize("domain", ["l1", "l2", "linf", "simplex"])
def test_hard_generator(apps, domain):
    import accbpg_and_fw_amd as acc
    m, n, R0 = 40, 12, 2.0
    out = apps.hard_FW_log_reg_jax(5, m, n, radius=R0, domain=domain, flip_y=0.1)
    f, h, L, L0, L1, x0, X, y = out
    assert isinstance(f, Recorded) and f.X is X and f.y is y and isinstance(h, acc.SquaredL2Norm)
    assert X.shape == (m, n) and y.shape == (m,) and x0.shape == (n,) and set(np.unique(y)) <= {-1.0, 1.0}
    assert L == L1 ** 2 and L1 == np.max(np.linalg.norm(X, axis=1)) and L0 == 1e-12
    assert np.array_equal(x0, np.zeros(n))                     # the centre: inside every ball; the reference's choice
    again = apps.hard_FW_log_reg_jax(np.random.RandomState(5), m, n, radius=R0, domain=domain, flip_y=0.1)
    assert np.array_equal(again[6], X) and np.array_equal(again[7], y) and np.array_equal(again[5], x0)
    other = apps.hard_FW_log_reg_jax(6, m, n, radius=R0, domain=domain, flip_y=0.1)
    assert not np.array_equal(other[6], X)
    # the columns carry the scales col_scale^linspace(0, 1, n) over Toeplitz-correlated rows
    plain = apps.hard_FW_log_reg_jax(5, m, n, radius=R0, domain=domain, col_scale=1.0)[6]
    np.testing.assert_allclose(X, plain * (10.0 ** np.linspace(0, 1, n))[None, :], rtol=1e-14)
    if domain in ("l1", "simplex"):
        v = apps.hard_FW_log_reg_jax(5, m, n, radius=R0, domain=domain, x0_mode="vertex")[5]
        assert np.count_nonzero(v) == 1 and v.sum() == R0 and np.all(v >= 0)


def test_older_generator(apps, capsys):
    m, n, R0 = 30, 6, 3.0
    f, h, L, L0, L1, x0 = apps.L0L1_FW_log_reg(7, m, n, R0)
    assert "true omega radius is" in capsys.readouterr().out
    assert f.X.shape == (m, n) and set(np.unique(f.y)) <= {-1.0, 1.0} and np.all(x0 == 1e-6)
    assert np.linalg.norm(x0) <= R0 and L == L1 ** 2 and L1 == np.max(np.linalg.norm(f.X, axis=1)) and L0 == 1e-9
    again = apps.L0L1_FW_log_reg(7, m, n, R0)
    assert np.array_equal(again[0].X, f.X) and np.array_equal(again[0].y, f.y)
    ratio = np.std(f.X, axis=0)
    assert ratio[-1] > 50 * ratio[0]                            # column j carries 3^j


def write_libsvm(path, X, labels):
    with open(path, "w") as fh:
        for row, lab in zip(X, labels):
            fh.write("%d %s\n" % (lab, " ".join("%d:%r" % (j + 1, float(v)) for j, v in enumerate(row) if v != 0)))


def test_a9a_loader_and_factory(apps, tmp_path):
    rng = np.random.RandomState(3)
    X = np.round(rng.rand(25, 7) * (rng.rand(25, 7) < 0.6), 3)
    X[:, 6] = rng.rand(25) + 0.1                                # the last column is dense: the width is 7
    labels = rng.choice([-1, 1], size=25)
    path = str(tmp_path / "small.libsvm")
    write_libsvm(path, X, labels)
    Xl, yl = apps.load_a9a_data(path)
    assert Xl.shape == (25, 8) and np.array_equal(Xl[:, :7], X) and np.all(Xl[:, 7] == 1.0)
    assert np.array_equal(yl, labels) and apps.load_a9a_data(path, bias=False)[0].shape == (25, 7)
    write_libsvm(path, X, (labels + 1) // 2)                    # labels 0 / 1 map to -1 / +1
    assert np.array_equal(apps.load_a9a_data(path)[1], labels)
    np.random.seed(11)
    f, h, L, L0, L1, x0 = apps.L0L1_FW_log_reg_a9a(0.3, path)
    Z = f.X
    np.testing.assert_allclose(Z[:, :7].mean(axis=0), 0.0, atol=1e-14)
    np.testing.assert_allclose(Z[:, :7].std(axis=0), 1.0, rtol=1e-13)
    np.testing.assert_allclose(Z[:, :7], (X - X.mean(axis=0)) / X.std(axis=0), rtol=1e-12, atol=1e-14)
    assert np.all(Z[:, 7] == 0.0)                               # the bias column: zero variance, scale 1
    assert x0.shape == (8,) and np.linalg.norm(x0) <= 0.3 and np.max(np.abs(x0)) <= 0.3
    assert L == L1 ** 2 and L1 == np.max(np.linalg.norm(Z, axis=1)) and L0 == 1e-9
    # a constant feature column as well
    Xc = X.copy()
    Xc[:, 2] = 4.0
    write_libsvm(path, Xc, labels)
    Zc = apps.L0L1_FW_log_reg_a9a(0.3, path)[0].X
    assert np.all(np.isfinite(Zc)) and np.all(Zc[:, 2] == 0.0) and np.all(Zc[:, 7] == 0.0)
    np.testing.assert_allclose(Zc[:, 3:7], Z[:, 3:7], rtol=1e-12, atol=1e-14)
