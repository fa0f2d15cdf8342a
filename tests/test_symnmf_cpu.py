"""CPU tests of the symmetric-NMF surface: exports with the reference's names and defaults (accbpg/functions.py:
493-577, 738-759, 908-976; accbpg/functions_lmo.py:16-51, 106-134; accbpg/algorithms_fw.py:210-247;
accbpg/applications.py:330-415), the C-ABI declarations, the Makefile flags of the new kernels, the NumPy
restatement (tests/symnmf_numpy.py) against the fixture written by the real reference (tools/gen_golden_symnmf.py),
and the factories' legacy-RNG draws on the host."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import symnmf_numpy as S  # noqa: E402

RADIUS = 500.0
INSTANCES = [("l2_400", "l2", 400, 50, 1), ("linf_400", "linf", 400, 50, 2), ("linf_700", "linf", 700, 50, 3)]
NEW_SYMBOLS = ["accbpg_symnmf_create", "accbpg_symnmf_destroy", "accbpg_symnmf_set_stream", "accbpg_symnmf_func_grad",
               "accbpg_symnmf_plan", "accbpg_quartic_prox_stage", "accbpg_quartic_ls_terms", "accbpg_lmo_l2_ball",
               "accbpg_lmo_linf_ball"]
E = inspect.Parameter.empty


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def cs(a):
    a = np.asarray(a, dtype=np.float64)
    return np.array([a.sum(), np.abs(a).sum(), (a * a).sum()])


def test_exports_and_signatures():
    import accbpg_and_fw_amd as acc
    for name in ["FrobeniusSymLoss", "SumOf2nd4thPowers", "SumOf2nd4thPowersPositiveOrthant", "SquaredL2Norm",
                 "FW_alg_descent_step", "lmo_l2_ball", "lmo_linf_ball", "FrobeniusSymLossExL2Ball",
                 "FrobeniusSymLossExLInfBall", "FrobeniusSymLossResMeasEx"]:
        assert name in acc.__all__ and hasattr(acc, name), name
    assert _sig(acc.FrobeniusSymLoss.__init__) == [("self", E), ("M", E), ("X_init", E), ("noise_level", None)]
    assert _sig(acc.FrobeniusSymLoss.func_grad) == [("self", E), ("X", E), ("flag", 2)]
    assert issubclass(acc.FrobeniusSymLoss, acc.RSmoothFunction)
    assert _sig(acc.SumOf2nd4thPowers.__init__) == [("self", E), ("alpha", E), ("sigma", E)]
    assert _sig(acc.SumOf2nd4thPowersPositiveOrthant.__init__) == [("self", E), ("alpha", E), ("sigma", E),
                                                                   ("upper_bound", None)]
    for cls in (acc.SumOf2nd4thPowers, acc.SumOf2nd4thPowersPositiveOrthant, acc.SquaredL2Norm):
        assert issubclass(cls, acc.LegendreFunction)
        assert _sig(cls.div_prox_map) == [("self", E), ("y", E), ("g", E), ("L", E)]
        assert _sig(cls.divergence) == [("self", E), ("x", E), ("y", E)]
    assert _sig(acc.SumOf2nd4thPowers.solve_cubic) == [("self", E), ("c", E), ("alpha", E)]
    assert _sig(acc.lmo_l2_ball) == [("radius", E), ("center", None)]
    assert _sig(acc.lmo_linf_ball) == [("radius", E), ("center", None)]
    assert _sig(acc.FW_alg_descent_step) == [("f", E), ("h", E), ("x0", E), ("maxitrs", E), ("lmo", E),
                                             ("epsilon", 1e-14), ("verbose", True), ("verbskip", 1)]
    for fac in (acc.FrobeniusSymLossExL2Ball, acc.FrobeniusSymLossExLInfBall):
        assert _sig(fac) == [("n", E), ("r", E), ("ball_center", E), ("radius", 1.0), ("on_boundary", True)]
    assert _sig(acc.FrobeniusSymLossResMeasEx) == [("M", E), ("r", E), ("noise", 0.0)]


def test_header_and_ctypes_table_carry_new_symbols():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.accbpg_abi_version() == 3
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_SYMBOLS:
        assert name in doc, name


def test_makefile_builds_new_kernels_without_contraction():
    mk = open(os.path.join(ROOT, "accbpg_and_fw_amd", "csrc", "Makefile")).read()
    for unit in ("symnmf_kernels", "quartic_kernels"):
        assert "build/%s.o" % unit in mk
        assert re.search(r"EXTRA_%s\s*=\s*-ffp-contract=off" % unit, mk), unit


def _instance(kind, n, r, seed):
    np.random.seed(seed)
    c = np.ones((n, r)) * RADIUS
    M, X0 = (S.l2_instance if kind == "l2" else S.linf_instance)(n, r, c, RADIUS, False)
    return M, X0, c


@pytest.mark.parametrize("tag,kind,n,r,seed", INSTANCES)
def test_factories_draw_the_reference_instance_on_the_host(tag, kind, n, r, seed):
    from accbpg_and_fw_amd import applications as A
    gd = golden("symnmf")
    M, X0, c = _instance(kind, n, r, seed)
    np.random.seed(seed)
    Mh, X0h = (A._symnmf_l2_instance if kind == "l2" else A._symnmf_linf_instance)(n, r, c, RADIUS, False)
    assert np.array_equal(M, Mh) and np.array_equal(X0, X0h)
    np.testing.assert_allclose(cs(Mh), gd[tag + "_M_cs"], rtol=1e-13)
    assert 2 * np.linalg.norm(Mh, 2) == pytest.approx(float(gd[tag + "_sigma"]), rel=1e-13)
    # the same generator state afterwards: later draws of a seeded script stay aligned
    np.random.seed(seed)
    (A._symnmf_l2_instance if kind == "l2" else A._symnmf_linf_instance)(n, r, c, RADIUS, False)
    after = np.random.rand()
    _instance(kind, n, r, seed)
    assert np.random.rand() == after


@pytest.mark.parametrize("tag,kind,n,r,seed", INSTANCES)
def test_restatement_reproduces_reference(tag, kind, n, r, seed):
    gd = golden("symnmf")
    M, X0, c = _instance(kind, n, r, seed)
    f = S.FrobeniusSymLoss(M, X0)
    h = S.SumOf2nd4thPowers(6, 2 * np.linalg.norm(M, 2))
    assert f(X0) == gd[tag + "_x0_f"]
    rng = np.random.RandomState(1000 + seed)
    X, G = rng.rand(n, r) * 2 * RADIUS, rng.randn(n, r) * 1e9
    fx, g = f.func_grad(X)
    assert fx == gd[tag + "_xr_f"]
    np.testing.assert_array_equal(g[:4], gd[tag + "_xr_g_rows"])
    np.testing.assert_array_equal(h.div_prox_map(X, G, 1e3)[:4], gd[tag + "_prox_q_1_rows"])
    ho = S.SumOf2nd4thPowersPositiveOrthant(h.alpha, h.sigma, upper_bound=RADIUS)
    np.testing.assert_array_equal(ho.div_prox_map(X, G, 1e6)[:4], gd[tag + "_prox_qu_2_rows"])
    np.testing.assert_array_equal([h.divergence(X, X0), h.divergence(X0, X)], gd[tag + "_div"])
    lmo = (S.lmo_l2_ball if kind == "l2" else S.lmo_linf_ball)(RADIUS, c)
    np.testing.assert_array_equal(lmo(G)[:4], gd[tag + "_lmo_g_rows"])
    nm2 = np.linalg.norm(M) ** 2
    for order in (0, 1):
        fo = S.FrobeniusSymLoss(M, X0, order=order)
        x, F, Ls = S.FW_alg_div_step(fo, h, 1, X0, 200, 2.0, lmo, ls_ratio=2.0)
        assert len(F) == len(gd[tag + "_fwls_F"])
        assert np.max(np.abs(F - gd[tag + "_fwls_F"])) <= 1e-12 * nm2
        np.testing.assert_array_equal(Ls, gd[tag + "_fwls_Ls"])
        x, F = S.FW_alg_descent_step(fo, h, X0, 200, lmo)
        assert np.max(np.abs(F - gd[tag + "_desc_F"])) <= 1e-12 * nm2


def test_restatement_lmo_edge_cases():
    g = np.zeros((3, 2))
    assert np.array_equal(S.lmo_l2_ball(2.0, center=1)(g), np.ones((3, 2)))
    g[0, 0] = -1.0
    s = S.lmo_linf_ball(2.0, center=1)(g)
    assert s[0, 0] == 3.0 and s[1, 1] == 1.0
