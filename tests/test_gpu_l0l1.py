"""GPU tests of FW_alg_L0_L1_shortest_step, FW_l0l1_log_and_linear_step and FW_l0l1_log_only on LogisticRegression
against the goldens of the real reference (tests/golden/l0l1.npz; nine runs of 60 iterations on the (120, 60) instance
of tests/l0l1_numpy.py), and of the three routes through an iteration against each other.

Against the goldens: the length, the number of trials and LOG_STEPS exactly, F to 1e-9, x within the reference's own
spread + 1e-12.  Ls = L0 + L1 ||g|| carries the rounding of the device's gradient (another summation order than
NumPy's), so it cannot have the golden's bits; it is held to 1e-9 like F, and exactly where two device routes compute
the same gradient.

fused=True against fused=False: assert_array_equal on x, F, Ls and LOG_STEPS -- the fused direction step has the bits
of the composition (tests/test_gpu_fw_direction.py).

carry=True against carry=False on the golden instances, where every acceptance test is decided by more than 1000 times
the carried-value bound (min_margin, asserted by the generator and by tests/test_l0l1_cpu.py): the trial counts and
LOG_STEPS are equal, and F[k] lies within k * value_step_bound + the epilogue's allowance of the uncarried F[k].  With
refresh=1 every iteration starts from a full func_grad, only the trial values are carried, and as no decision flips the
whole run -- x, F, Ls, LOG_STEPS -- is the uncarried one bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import l0l1_numpy as LL  # noqa: E402
from conftest import golden  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(s, d) for s in LL.SOLVERS for d in LL.DOMAINS]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def gold():
    return golden("l0l1")


class Counting:
    """the objective with its value-only calls counted: func_grad(., flag=0) and line_value"""

    def __init__(self, f):
        self._f, self.values, self.full, self.carried = f, 0, 0, 0

    def func_grad(self, x, flag=2):
        self.values += flag == 0
        self.full += flag != 0
        return self._f.func_grad(x, flag)

    def line_value(self, a):
        self.values += 1
        return self._f.line_value(a)

    def func_grad_carried(self, flag=2):
        self.carried += 1
        return self._f.func_grad_carried(flag)

    def __getattr__(self, name):
        return getattr(self._f, name)


@pytest.fixture(scope="module")
def problem(acc, gold):
    A, y = LL.instance()
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["A_checksum"], rtol=1e-14)
    return A, y, acc.LogisticRegression(A, y)


def solve(acc, problem, solver, domain, x0=None, **extra):
    A, y, f = problem
    lmo = {"l2": acc.lmo_l2_ball, "linf": acc.lmo_linf_ball, "simplex": acc.lmo_simplex}[domain](LL.RADIUS[domain])
    cf = Counting(f)
    x0 = LL.start(domain, A.shape[1]) if x0 is None else x0
    out = LL.call_solver(acc, solver, cf, acc.SquaredL2Norm(), x0, lmo, LL.run_params(solver, domain, A), **extra)
    return out, cf


@pytest.fixture(scope="module")
def plain(acc, problem):
    """the uncarried fused runs, computed once"""
    return {case: solve(acc, problem, *case) for case in CASES}


@pytest.mark.parametrize("solver,domain", CASES)
def test_whole_runs_against_goldens(gold, plain, solver, domain):
    key = "%s_%s" % (solver, domain)
    (x, F, Ls, LOG), cf = plain[(solver, domain)]
    Fr, Lr = gold[key + "_F"], gold[key + "_Ls"]
    assert isinstance(x, np.ndarray) and len(F) == len(Fr) == len(Ls)
    dF = np.abs(F - Fr) / (1 + np.abs(Fr))
    dx = float(np.max(np.abs(x - gold[key + "_x"])))
    print("%s: trials %d  max dF %.2e  max dLs %.2e  dx %.2e (spread %.2e)" % (
        key, cf.values, dF.max(), float(np.max(np.abs(Ls - Lr) / Lr)), dx, float(gold[key + "_xspread"])))
    assert cf.values == int(gold[key + "_trials"]) and cf.full == len(F) and cf.carried == 0
    if LOG is not None:
        assert np.array_equal(LOG, gold[key + "_LOG"])
    assert np.all(dF <= 1e-9)
    np.testing.assert_allclose(Ls, Lr, rtol=1e-9)
    assert dx <= float(gold[key + "_xspread"]) + 1e-12


@pytest.mark.parametrize("solver,domain", CASES)
def test_fused_is_the_composition_bit_for_bit(acc, problem, plain, solver, domain):
    (x, F, Ls, LOG), cf = plain[(solver, domain)]
    (x2, F2, Ls2, LOG2), cf2 = solve(acc, problem, solver, domain, fused=False)
    np.testing.assert_array_equal(x2, x)
    np.testing.assert_array_equal(F2, F)
    np.testing.assert_array_equal(Ls2, Ls)
    assert cf2.values == cf.values
    if LOG is not None:
        np.testing.assert_array_equal(LOG2, LOG)


def test_foreign_oracle_and_tensor_in_tensor_out(acc, problem, plain):
    A, y, f = problem
    (x, F, Ls, LOG), _ = plain[("loglin", "linf")]
    # an oracle the package does not know goes through the composition: the same run
    inner = acc.lmo_linf_ball(LL.RADIUS["linf"])
    out = acc.FW_l0l1_log_and_linear_step(f, acc.SquaredL2Norm(), *LL.constants(A), np.zeros(A.shape[1]), LL.ITERS,
                                          lambda g: inner(g), 2.0, verbose=False)
    np.testing.assert_array_equal(out[0], x)
    np.testing.assert_array_equal(out[1], F)
    np.testing.assert_array_equal(out[3], LOG)
    # CUDA tensor in, CUDA tensor out
    x0 = torch.zeros(A.shape[1], dtype=torch.float64, device="cuda")
    for kw in (dict(), dict(fused=False), dict(carry=True)):
        out = acc.FW_l0l1_log_and_linear_step(f, acc.SquaredL2Norm(), *LL.constants(A), x0, LL.ITERS, inner, 2.0,
                                              verbose=False, **kw)
        assert isinstance(out[0], torch.Tensor) and out[0].is_cuda and torch.count_nonzero(x0) == 0
        assert isinstance(out[1], np.ndarray) and len(out) == 5
        if not kw.get("carry"):
            np.testing.assert_array_equal(out[0].cpu().numpy(), x)
    out = acc.FW_alg_L0_L1_shortest_step(f, acc.SquaredL2Norm(), *LL.constants(A), x0, 5, 2.0, inner, verbose=False)
    assert isinstance(out[0], torch.Tensor) and len(out) == 4 and len(out[1]) == 5


@pytest.mark.parametrize("solver,domain", CASES)
def test_carried_margins_take_the_same_decisions(acc, gold, problem, plain, solver, domain):
    A = problem[0]
    key = "%s_%s" % (solver, domain)
    (x, F, Ls, LOG), cf = plain[(solver, domain)]
    step = LL.value_step_bound(A, domain)
    allow = 2 * LL.LN.T_ULP * LL.LN.U * float(np.max(F))
    assert float(gold[key + "_min_margin"]) > 1000 * ((LL.REFRESH - 1) * step + allow)
    (xc, Fc, Lc, LOGc), cc = solve(acc, problem, solver, domain, carry=True)
    assert len(Fc) == len(F) and cc.values == cf.values and cc.full == 1 and cc.carried == len(F) - 1
    if LOG is not None:
        np.testing.assert_array_equal(LOGc, LOG)
    dF = np.abs(Fc - F)
    bound = np.arange(len(F)) * step + allow
    print("%s: carried max |dF| %.2e, at most %.2e of its bound; max dLs %.2e; dx %.2e" % (
        key, dF.max(), float(np.max(dF / bound)), float(np.max(np.abs(Lc - Ls) / Ls)), float(np.max(np.abs(xc - x)))))
    assert np.all(dF <= bound)
    np.testing.assert_allclose(Lc, Ls, rtol=1e-9)               # (the carried gradient has its own rounding)
    # refresh = 1: only the trial values are carried, and no decision flips: the same run bit for bit
    (x1, F1, L1, LOG1), c1 = solve(acc, problem, solver, domain, carry=True, refresh=1)
    assert c1.values == cf.values and c1.full == len(F) and c1.carried == 0
    np.testing.assert_array_equal(x1, x)
    np.testing.assert_array_equal(F1, F)
    np.testing.assert_array_equal(L1, Ls)
    if LOG is not None:
        np.testing.assert_array_equal(LOG1, LOG)


def test_refresh_in_between_and_the_d_zero_ending(acc, problem, plain):
    A, y, f = problem
    (x, F, Ls, LOG), cf = plain[("logonly", "l2")]
    (x7, F7, L7, LOG7), c7 = solve(acc, problem, "logonly", "l2", carry=True, refresh=7)
    assert c7.full == len(range(0, LL.ITERS, 7)) and c7.carried == LL.ITERS - c7.full and c7.values == cf.values
    np.testing.assert_array_equal(LOG7, LOG)
    assert np.all(np.abs(F7 - F) <= 7 * LL.value_step_bound(A, "l2") + 6 * LL.LN.U)
    # an oracle that answers x itself: the run ends at that iteration with the traces so far
    for kw in (dict(), dict(carry=True)):
        out = acc.FW_l0l1_log_only(f, acc.SquaredL2Norm(), 1.0, 1.0, np.full(A.shape[1], 0.01), 10,
                                   lambda g: torch.full_like(g, 0.01), 2.0, verbose=False, **kw)
        assert len(out[1]) == 1 and len(out[2]) == 0 and out[3].tolist() == [0] and np.all(out[0] == 0.01)
