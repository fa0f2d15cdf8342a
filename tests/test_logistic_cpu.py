"""CPU tests of the logistic family: the C-ABI and Python names, the measurement behind the allowances T_ULP and Q_ULP,
the float64 NumPy restatement (tests/logistic_numpy.py) inside every forward bound at every shape of the GPU module,
the restatement against the goldens the real reference wrote (tests/golden/logistic.npz,
tools/gen_golden_logistic.py), and the reach of the GPU module's shape list.

L2L1Linf is elementwise IEEE arithmetic, so the restatement must have the reference's bits; its two sums (extra_Psi,
divergence) are NumPy's pairwise sums on both sides, also bit for bit.  Whole runs: F to 1e-9 over the stored length,
x within the reference's own spread under a 4e-16 perturbation of its margins + 1e-12, G to 1e-9 relative."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_numpy as LN  # noqa: E402
import reduce_numpy as T  # noqa: E402
from conftest import golden  # noqa: E402
from accbpg_and_fw_amd import L2L1Linf, Logistic_regr_L2L1Linf, LogisticRegression  # noqa: E402,F401  (the feature)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["accbpg_logistic_create", "accbpg_logistic_destroy", "accbpg_logistic_set_stream",
               "accbpg_logistic_func_grad", "accbpg_logistic_get", "accbpg_l2l1linf_prox", "accbpg_l1_norm",
               "accbpg_sq_ls_terms"]


@pytest.fixture(scope="module")
def gold():
    return golden("logistic")


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


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
    for name in ("LogisticRegression", "L2L1Linf", "Logistic_regr_L2L1Linf"):
        assert name in acc.__all__ and hasattr(acc, name)
    assert list(inspect.signature(acc.LogisticRegression.__init__).parameters) == ["self", "X", "y", "alpha"]
    assert inspect.signature(acc.LogisticRegression.__init__).parameters["alpha"].default == 0.01
    sig = inspect.signature(acc.L2L1Linf.__init__).parameters
    assert list(sig) == ["self", "lamda", "B"] and sig["lamda"].default == 0 and sig["B"].default == 1
    sig = inspect.signature(acc.Logistic_regr_L2L1Linf).parameters
    assert list(sig) == ["m", "n", "lamda", "B", "randseed", "labels"]
    assert [sig[k].default for k in ("lamda", "B", "randseed", "labels")] == [None, 1, -1, None]
    assert inspect.signature(acc.LogisticRegression.func_grad).parameters["flag"].default == 2
    for name in ("f", "__call__", "gradient", "func_grad", "fitted", "losses", "weights"):
        assert hasattr(acc.LogisticRegression, name)
    for name in ("__call__", "extra_Psi", "gradient", "divergence", "prox_map", "div_prox_map", "ls_terms"):
        assert hasattr(acc.L2L1Linf, name)
    from accbpg_and_fw_amd.algorithms import _divergences
    assert "L2L1Linf" in inspect.getsource(_divergences)


def test_allowances_are_the_measured_ones():
    """NumPy's fp64 t and q against np.longdouble over 20 000 exact-data margins and the planted values; the
    np.longdouble reference against mpmath at 40 digits on the planted values and a sample"""
    s = LN.measured_margins()
    assert s.size >= 20000
    t_err, q_err = LN.measure_tq(s)
    print("measured: t %.3f ulp, q %.3f ulp over %d margins" % (t_err, q_err, s.size))
    assert t_err <= LN.T_MEASURED and q_err <= LN.Q_MEASURED
    assert LN.T_ULP == int(np.ceil(LN.T_MEASURED)) + 1 and LN.Q_ULP == int(np.ceil(LN.Q_MEASURED)) + 1
    pytest.importorskip("mpmath")
    fin = [v for v in LN.PLANTED_S if np.isfinite(v)] + list(s[np.isfinite(s)][100:140])
    tr, qr = LN.tq_ref(np.array(fin))
    for i, v in enumerate(fin):
        tm, qm = LN.tq_mp(v)
        # the np.longdouble evaluation itself: within 4 of its own ulps (2^-63 relative), or one subnormal double
        assert abs(tr[i] - tm) <= 4 * 2.0 ** -63 * abs(tm) + LN.TINY, (v, tr[i], tm)
        assert abs(qr[i] - qm) <= 4 * 2.0 ** -63 * abs(qm) + LN.TINY, (v, qr[i], qm)


def test_special_margins_of_the_restatement():
    s = np.array(LN.PLANTED_S)
    t, q = LN.tq_fp64(s)
    at = {v: i for i, v in enumerate(LN.PLANTED_S) if v == v and v != 0}
    assert t[0] == np.log1p(1.0) and t[1] == t[0] and q[0] == 0.5 and q[1] == 0.5
    for v in (746.0, 1e4, np.inf):
        assert t[at[v]] == 0.0 and q[at[v]] == 0.0 and t[at[-v]] == v and q[at[-v]] == 1.0
    assert np.isnan(t[-1]) and np.isnan(q[-1])
    assert 0 < t[at[745.0]] <= 2 * LN.TINY and t[at[-745.0]] == 745.0
    # rows: r = -(y*q); a NaN label gives NaN t and r
    tt, rr = LN.epilogue(np.array([0.0, 1.0, 1.0]), np.array([-1.0, np.nan, -np.inf]))
    assert rr[0] == 0.5 and np.isnan(tt[1]) and np.isnan(rr[1]) and tt[2] == np.inf and rr[2] == np.inf


@pytest.mark.parametrize("m,n", LN.EXACT_SHAPES)
def test_restatement_inside_every_bound_on_exact_data(m, n):
    A, x, y = LN.exact_data(m, n, 100 * m + n)
    z = A.dot(x)
    assert same_bits(z, np.asarray(A, dtype=LN.LD).dot(np.asarray(x, dtype=LN.LD)).astype(np.float64))   # exact
    t, r = LN.epilogue(z, y)
    ref = LN.refs_and_bounds(A, z, y)
    assert np.all(np.abs(LN.LD(t) - ref["t"]) <= ref["t_bound"])
    assert np.all(np.abs(LN.LD(r) - ref["r"]) <= ref["r_bound"])
    f = T.tree_sum(t, T.CAP_VEC) / m
    g = np.dot(r, A) / m
    assert abs(LN.LD(f) - ref["f"]) <= ref["f_bound"]
    assert np.all(np.abs(LN.LD(g) - ref["g"]) <= ref["g_bound"])
    f2, g2 = LN.LogisticRegression(A, y).func_grad(x, 2)
    assert abs(LN.LD(f2) - ref["f"]) <= ref["f_bound"] and same_bits(g2, g)


def test_bounds_are_tight_enough_to_see_a_wrong_formula():
    """the unstable textbook forms miss the row bounds on the planted values"""
    s = np.array([36.0, 37.0, 50.0, -50.0])
    tr, qr = LN.tq_ref(s)
    with np.errstate(all="ignore"):
        naive_t = np.log(1 + np.exp(-s))
    assert np.any(np.abs(LN.LD(naive_t) - tr) > LN.ulps(LN.T_ULP, tr))
    t, q = LN.tq_fp64(s)
    assert np.all(np.abs(LN.LD(t) - tr) <= LN.ulps(LN.T_ULP, tr))
    assert np.all(np.abs(LN.LD(q) - qr) <= LN.ulps(LN.Q_ULP, qr))


def gauss(gold):
    A, y = LN.gaussian_instance()
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["gauss_A_checksum"], rtol=1e-14)
    assert np.array_equal(y, gold["gauss_y"]) and set(y) == {-1.0, 1.0}
    return A, y


def test_percall_goldens_inside_the_general_data_bounds(gold):
    """The stored f and g come from the generator's own objective (np.logaddexp and scipy's expit), not from the
    restatement: both are float64 evaluations and both must lie inside the general-data bounds around the
    np.longdouble reference, with the chain length of a NumPy dot product (n) in the place of the device's.  The
    independent evidence of this module is that reference, mpmath behind it, and the real reference's L2L1Linf and
    solvers; the stored A x is NumPy's own dot product and is compared bit for bit only to pin the instance."""
    A, y = gauss(gold)
    pts = gold["pc_x"]
    assert same_bits(pts, LN.box_points(A.shape[1])) and np.max(np.abs(pts)) <= 1.0
    f = LN.LogisticRegression(A, y)
    for i, x in enumerate(pts):
        z = gold["pc_Ax"][i]
        assert same_bits(z, A.dot(x))
        zl = np.asarray(A, dtype=LN.LD).dot(np.asarray(x, dtype=LN.LD))
        ds = LN.ds_bound(A, x, y, y * z, chain=A.shape[1])
        assert np.all(np.abs(LN.LD(z) - zl) <= ds)
        ref = LN.refs_and_bounds(A, zl.astype(np.float64), y, ds=ds + LN.U * np.abs(zl))
        for v, g in ((gold["pc_f"][i], gold["pc_g"][i]), f.func_grad(x, 2)):
            assert abs(LN.LD(v) - ref["f"]) <= ref["f_bound"]
            assert np.all(np.abs(LN.LD(g) - ref["g"]) <= ref["g_bound"])


def test_l2l1linf_restatement_has_the_reference_bits(gold):
    A, y = gauss(gold)
    pts, m = gold["pc_x"], A.shape[0]
    assert same_bits(gold["k_lamda"], [0.0, 1.0 / m, 0.3]) and same_bits(gold["k_L"], LN.KERNEL_L)
    for a, lamda in enumerate(gold["k_lamda"]):
        h = LN.L2L1Linf(lamda=float(lamda), B=1)
        for i, x in enumerate(pts):
            g = gold["pc_g"][i]
            assert same_bits(h.extra_Psi(x), gold["k_psi"][a, i])
            assert same_bits(h.divergence(x, pts[(i + 1) % 3]), gold["k_div"][i]) and same_bits(h(x), gold["k_h"][i])
            for b, L in enumerate(gold["k_L"]):
                assert same_bits(h.prox_map(g, float(L)), gold["k_prox"][a, b, i])
                assert same_bits(h.div_prox_map(x, g, float(L)), gold["k_dprox"][a, b, i])
    # both branches of the threshold and the clip occur in the stored values
    assert np.any(gold["k_prox"] == 0) and np.any(np.abs(gold["k_prox"]) == 1) and np.any(
        (gold["k_dprox"] != 0) & (np.abs(gold["k_dprox"]) < 1))


RUN_NAMES = list(LN.run_table(LN.SOLVERS, LN.lmo_linf_ball))


def run_instance(gold):
    A, b = LN.example_draws()
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["run_A_checksum"], rtol=1e-14)
    assert np.all(b == 1.0) and b.shape == (A.shape[0], 1)
    y = LN.example_labels()
    assert np.array_equal(y, gold["run_y"])
    return A, y


@pytest.mark.parametrize("name", RUN_NAMES)
def test_runs_restatement_equals_goldens(gold, name):
    A, y = run_instance(gold)
    m, n = A.shape
    f = LN.LogisticRegression(A, y)
    h, sh = LN.L2L1Linf(lamda=float(gold["run_lamda"]), B=float(gold["run_B"])), LN.SquaredL2Norm()
    assert float(gold["run_lamda"]) == 1.0 / m and float(gold["run_L"]) == 0.25
    key = "run_" + name
    assert int(gold[key + "_prefix"]) == len(gold[key + "_F"]) == LN.ITERS
    x, F, G = LN.run_table(LN.SOLVERS, LN.lmo_linf_ball)[name](f, h, sh, 0.25, np.zeros(n), float(gold["run_B"]))
    assert len(F) == len(gold[key + "_F"])
    assert np.all(np.abs(F - gold[key + "_F"]) <= 1e-9 * (1 + np.abs(gold[key + "_F"])))
    assert np.max(np.abs(x - gold[key + "_x"])) <= float(gold[key + "_xspread"]) + 1e-12
    np.testing.assert_allclose(G, gold[key + "_G"], rtol=1e-9)
    assert F[-1] < F[0] and np.max(np.abs(x)) <= float(gold["run_B"])


def test_launch_forms_are_all_reached():
    """with 256 compute units the shapes of the GPU module cover every selecting condition of pass 1 and every regime
    of vt_nsplit in pass 2"""
    cu = 256
    shapes = LN.all_shapes()
    forms = {s: LN.ax_form(s[0], s[1], cu) for s in shapes}
    assert forms[(33, 4096)] == "wg" and forms[(5, 4097)] == "wg"
    assert forms[LN.LONG_SHAPE] == "hold"
    wave = [s for s in shapes if forms[s] == "wave"]
    assert any(m >= 8 * cu for m, n in wave) and any(n < 4096 and m < 8 * cu for m, n in wave)
    splits = {s: LN.vt_nsplit(s[0], s[1], cu) for s in shapes}
    assert any(v == 1 for v in splits.values())
    assert any(v == s[0] // 8 and 1 < v < 64 for s, v in splits.items()), splits          # the m/8 cap
    assert any(1 < v < min(64, s[0] // 8) for s, v in splits.items()), splits             # in between
    assert any(v == 64 for v in splits.values()), splits                                  # the 64 cap
    # the sum of t: one block and several
    blocks = [T.red_blocks(m, T.CAP_VEC) for m, n in shapes]
    assert min(blocks) == 1 and max(blocks) > 1
    for m, n in LN.PLANTED_SHAPES:
        assert (m, n) in shapes


def test_factory_draws_equal_the_example():
    """the draws of Logistic_regr_L2L1Linf are those of ex_LR_L2L1Linf.py:61-63, in order (host arithmetic only: the
    generator's position is compared, no device is needed for that)"""
    A, b = LN.example_draws(12, 7, seed=5)
    after = np.random.random_sample()
    np.random.seed(5)
    A2 = np.random.randn(12, 7)
    b2 = np.sign(np.random.rand(12, 1))
    assert same_bits(A, A2) and same_bits(b, b2) and np.random.random_sample() == after
