"""CPU tests of the KL-divergence regression / Shannon-entropy surface: exports with the reference's names and
defaults (accbpg/functions.py:123-158, 398-490; accbpg/applications.py:175), the C-ABI declarations, and the NumPy
restatement (tests/kl_numpy.py) against the fixture written by the real reference (tools/gen_golden_kl.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kl_numpy as K  # noqa: E402

SIZES = [("s1", 1000, 100), ("s2", 100, 1000)]
ARGS = dict(noise=0.01, lamdaL1=0.001, randseed=1)
NEW_SYMBOLS = ["accbpg_kldiv_create", "accbpg_kldiv_destroy", "accbpg_kldiv_set_stream", "accbpg_kldiv_func_grad",
               "accbpg_kldiv_get_ax", "accbpg_shannon_div_prox", "accbpg_shannon_ls_terms",
               "accbpg_shannon_divergence"]


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_exports_and_signatures():
    import accbpg_and_fw_amd as acc
    E = inspect.Parameter.empty
    for name in ["KLdivRegression", "ShannonEntropy", "ShannonEntropyL1", "ShannonEntropySimplex", "KL_nonneg_regr"]:
        assert name in acc.__all__ and hasattr(acc, name), name
    assert _sig(acc.KL_nonneg_regr) == [("m", E), ("n", E), ("noise", 0.01), ("lamdaL1", 0), ("randseed", -1),
                                        ("normalizeA", True)]
    assert _sig(acc.KLdivRegression.__init__) == [("self", E), ("A", E), ("b", E)]
    assert _sig(acc.KLdivRegression.func_grad) == [("self", E), ("x", E), ("flag", 2)]
    assert _sig(acc.ShannonEntropy.__init__) == [("self", E), ("delta", 1e-20)]
    assert _sig(acc.ShannonEntropyL1.__init__) == [("self", E), ("lamda", 0), ("delta", 1e-20)]
    assert _sig(acc.ShannonEntropySimplex.__init__) == [("self", E), ("delta", 1e-20)]
    for cls in (acc.ShannonEntropy, acc.ShannonEntropyL1, acc.ShannonEntropySimplex):
        assert issubclass(cls, acc.LegendreFunction)
        assert _sig(cls.prox_map) == [("self", E), ("g", E), ("L", E)]
        assert _sig(cls.div_prox_map) == [("self", E), ("y", E), ("g", E), ("L", E)]
        assert _sig(cls.divergence) == [("self", E), ("x", E), ("y", E)]
    assert issubclass(acc.KLdivRegression, acc.RSmoothFunction)


def test_header_and_ctypes_table_carry_new_symbols():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.accbpg_abi_version() == 3


def test_makefile_builds_shannon_without_contraction():
    mk = open(os.path.join(ROOT, "accbpg_and_fw_amd", "csrc", "Makefile")).read()
    assert "build/shannon_kernels.o" in mk
    assert re.search(r"EXTRA_shannon_kernels\s*=\s*-ffp-contract=off", mk)


@pytest.mark.parametrize("tag,m,n", SIZES)
def test_restatement_reproduces_reference_percall(tag, m, n):
    gd = golden("kl")
    f, h, L, x0 = K.KL_nonneg_regr(m, n, **ARGS)
    assert np.array_equal(f.b, gd[tag + "_b"]) and L == gd[tag + "_L"]
    np.testing.assert_array_equal(x0, gd[tag + "_x0"])
    np.testing.assert_allclose([f.A.sum(), np.abs(f.A).max(), (f.A ** 2).sum()], gd[tag + "_A_checksum"], rtol=1e-13)
    x, y, g = gd[tag + "_x"], gd[tag + "_y"], gd[tag + "_g"]
    fx, gx = f.func_grad(x, 2)
    assert fx == pytest.approx(float(gd[tag + "_f"]), rel=1e-13)
    np.testing.assert_allclose(gx, g, rtol=1e-13, atol=1e-13)
    assert f(x0) == pytest.approx(float(gd[tag + "_f0"]), rel=1e-13)
    np.testing.assert_allclose(f.gradient(x0), gd[tag + "_g0"], rtol=1e-13, atol=1e-13)
    assert h.extra_Psi(x) == pytest.approx(float(gd[tag + "_psi"]), rel=1e-13)
    for kname, hk in [("sh", K.Shannon()), ("l1", K.ShannonL1(ARGS["lamdaL1"])), ("sx", K.ShannonSimplex())]:
        for idx, Lc in enumerate(gd[tag + "_prox_L"]):
            np.testing.assert_allclose(hk.prox_map(g, Lc), gd["%s_%s_prox%d" % (tag, kname, idx)], rtol=1e-13)
            np.testing.assert_allclose(hk.div_prox_map(y, g, Lc), gd["%s_%s_divprox%d" % (tag, kname, idx)],
                                       rtol=1e-13)
        assert hk.divergence(x, y) == pytest.approx(float(gd["%s_%s_div_xy" % (tag, kname)]), rel=1e-13)
        assert hk.divergence(gd[tag + "_xz"], gd[tag + "_yz"]) == \
            pytest.approx(float(gd["%s_%s_div_zero" % (tag, kname)]), rel=1e-13)


@pytest.mark.parametrize("tag,m,n", SIZES)
def test_restatement_reproduces_reference_trajectories(tag, m, n):
    """BPG (with and without line search) and ABPG of the notebook, 2000 iterations, through the solvers of
    oracle/np_oracle.py: the restatement carries the reference's operation order, so x, F and G agree to 1e-13."""
    from oracle import np_oracle as O
    gd = golden("kl")
    f, h, L, x0 = K.KL_nonneg_regr(m, n, **ARGS)
    N = 2000
    runs = {"bpg": lambda: O.BPG(f, h, L, x0, maxitrs=N, linesearch=False),
            "bpgls": lambda: O.BPG(f, h, L, x0, maxitrs=N, linesearch=True, ls_ratio=1.2),
            "abpg": lambda: O.ABPG(f, h, L, x0, gamma=2.0, maxitrs=N, theta_eq=True, restart=False)}
    for name, run in runs.items():
        x, F, G, _ = run()
        assert len(F) == len(gd["%s_%s_F" % (tag, name)]), name
        np.testing.assert_allclose(x, gd["%s_%s_x" % (tag, name)], rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(F, gd["%s_%s_F" % (tag, name)], rtol=1e-13)
        np.testing.assert_allclose(G, gd["%s_%s_G" % (tag, name)], rtol=1e-13)


def test_fixture_rows_match_the_notebook():
    """F of the printed rows of ex_KL_regr_L1.ipynb (k = 0, 1000, ..., 4000), as the fixture recorded them."""
    gd = golden("kl")
    printed = {("s1", "bpg"): ["3.079e-01", "1.287e-01", "1.280e-01", "1.279e-01", "1.278e-01"],
               ("s1", "abpg"): ["3.079e-01", "1.278e-01", "1.278e-01", "1.278e-01", "1.278e-01"],
               ("s2", "bpg"): ["5.275e-01", "4.988e-01", "4.987e-01", "4.987e-01", "4.987e-01"],
               ("s2", "gain"): ["5.275e-01", "4.987e-01", "4.987e-01", "4.987e-01"]}
    for (tag, name), rows in printed.items():
        got = ["%.3e" % v for v in gd["%s_%s_rows" % (tag, name)][:len(rows)]]
        assert got == rows, (tag, name)
    assert int(gd["s2_gainrs_len"]) == 299
