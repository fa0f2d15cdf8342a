"""Generate tests/golden/l0l1.npz by running the real reference's FW_alg_L0_L1_shortest_step,
FW_l0l1_log_and_linear_step and FW_l0l1_log_only with its lmo_l2_ball, lmo_linf_ball and lmo_simplex and its
SquaredL2Norm on the NumPy stand-in objective of tests/l0l1_numpy.py.

TEST INFRASTRUCTURE ONLY: runs on a machine that holds the reference, never on the GPU box.  The reference package is
imported read-only through oracle/gen_golden.load_reference and called on seeded inputs; only numbers are written.

Contents: for each of the nine runs (three solvers on the three domains, 60 iterations on the (120, 60) instance) x, F,
Ls, LOG_STEPS, the number of trials, `prefix` and `xspread` as tools/gen_golden_logistic.py defines them (three reruns
with the margins perturbed at relative 4e-16; every stored run must have prefix == len(F)), and `min_margin`, the
smallest |lhs - rhs| over the run's acceptance tests.  The reference does not expose the two sides of its tests, so
min_margin comes from the run objects of accbpg_and_fw_amd/solver_runs.py driven on the same objective -- after they
have reproduced the reference's run bit for bit.

The generator asserts what the tests rely on: a failed test on either toggle, a cap on L1 that binds, both kinds of
step in FW_l0l1_log_and_linear_step, and for every run min_margin > 1000 * (the carried-value bound of REFRESH - 1
steps), so that carried margins cannot flip a decision.

Usage:  python tools/gen_golden_l0l1.py
"""
import importlib.util
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

from oracle.gen_golden import load_reference, save  # noqa: E402
import l0l1_numpy as LL  # noqa: E402
from gen_golden_inexact import agree  # noqa: E402


def solver_runs():
    """accbpg_and_fw_amd/solver_runs.py on its own: it needs NumPy only, the package needs the GPU library"""
    spec = importlib.util.spec_from_file_location("solver_runs", os.path.join(ROOT, "accbpg_and_fw_amd", "solver_runs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_lmo(accbpg, domain):
    R = LL.RADIUS[domain]
    return {"l2": accbpg.lmo_l2_ball, "linf": accbpg.lmo_linf_ball, "simplex": accbpg.lmo_simplex}[domain](R)


def main():
    accbpg = load_reference()
    R = solver_runs()
    A, y = LL.instance()
    m, n = A.shape
    h = accbpg.SquaredL2Norm()
    out = {"A_checksum": np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()]), "y": y}
    seen = {"toggle0": False, "toggle1": False, "cap": False, "log": False, "linear": False}
    for solver in LL.SOLVERS:
        for domain in LL.DOMAINS:
            key = "%s_%s" % (solver, domain)
            params, x0 = LL.run_params(solver, domain, A), LL.start(domain, n)
            f = LL.StandIn(A, y)
            x, F, Ls, LOG = LL.call_solver(accbpg, solver, f, h, np.copy(x0), ref_lmo(accbpg, domain), params)
            assert np.all(np.isfinite(F)) and np.all(np.isfinite(Ls)) and len(F) == LL.ITERS, key
            prefix, xspread = len(F), 0.0
            for s in range(3):
                fp = LL.StandIn(A, y, perturb=np.random.RandomState(31 + s))
                xp, Fp, Lp, LOGp = LL.call_solver(accbpg, solver, fp, h, np.copy(x0), ref_lmo(accbpg, domain), params)
                assert len(Fp) == len(F), "%s: a perturbed rerun has another length: change the seed" % key
                assert LOG is None or np.array_equal(LOG, LOGp), "%s: a perturbed rerun takes other trials" % key
                assert fp.values == f.values, "%s: a perturbed rerun takes other trials: change the seed" % key
                prefix = min(prefix, agree(Fp, F, 1e-9), agree(Lp, Ls, 1e-9))
                xspread = max(xspread, float(np.max(np.abs(xp - x))))
            assert prefix == len(F), "%s reproduces itself on %d of %d iterations only: change the seed" % (
                key, prefix, len(F))
            # the run objects on the same objective: the reference's bits, and the two sides of every test
            tests, f2 = [], LL.StandIn(A, y)
            run = LL.make_run(R, solver, params)
            lmo = {"l2": LL.lmo_l2_ball, "linf": LL.lmo_linf_ball, "simplex": LL.lmo_simplex}[domain](LL.RADIUS[domain])
            res = LL.drive(run, f2, LL.SquaredL2Norm(), x0, LL.ITERS, lmo, solver == "shortest", tests)
            assert np.array_equal(res[0], x) and np.array_equal(res[1], F) and np.array_equal(res[2], Ls), key
            assert LOG is None or np.array_equal(res[3], LOG), key
            assert f2.values == f.values == len(tests)
            min_margin = min(abs(a - b) for a, b in tests)
            carried = (LL.REFRESH - 1) * LL.value_step_bound(A, domain) + 2 * LL.LN.T_ULP * LL.LN.U * float(np.max(F))
            assert min_margin > 1000 * carried, "%s: a test is decided by %.2e, the carried bound is %.2e" % (
                key, min_margin, carried)
            # what the runs must show between them
            fails = [i for i, (a, b) in enumerate(tests) if not a <= b]
            if solver != "loglin" and fails:
                seen["toggle0"] = True
                seen["toggle1"] = seen["toggle1"] or len(fails) >= 2
            if "L1_max" in params and run.L1 == params["L1_max"]:
                seen["cap"] = True
            if solver == "loglin":
                steps = np.diff(LOG)
                seen["log"] = seen["log"] or bool(np.any(steps == 1))
                seen["linear"] = seen["linear"] or bool(np.any(steps == 0))
            out.update({key + "_x": x, key + "_F": F, key + "_Ls": Ls, key + "_trials": f.values, key + "_prefix": prefix,
                        key + "_xspread": xspread, key + "_min_margin": min_margin, key + "_fails": len(fails)})
            if LOG is not None:
                out[key + "_LOG"] = LOG
            print("%-18s trials %3d (failed %2d) xspread %.2e min_margin %.2e (carried %.1e) F %.6e -> %.6e" % (
                key, f.values, len(fails), xspread, min_margin, carried, F[0], F[-1]), flush=True)
    assert all(seen.values()), seen
    save("l0l1", **out)


if __name__ == "__main__":
    main()
