"""CPU tests of the inexact-oracle surface: exports with the reference's names and defaults (accbpg/algorithms.py:
593-777; accbpg/applications.py:209-295; accbpg/utils.py:252-295; accbpg/functions_lmo.py:54), the C-ABI declarations,
the host-side helpers and factories' RNG call sequence, and the NumPy restatement (tests/inexact_numpy.py) against
the fixture written by the real reference (tools/gen_golden_inexact.py)."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inexact_numpy as R  # noqa: E402

SEED = 7
ACC = dict(m=2000, n=1000, noise=0.001)
ACC_ITERS = 80
FW = dict(m=300, n=500, noise=0.001)
RUN_SEED = 1991
NOISES = [0, 1e-6]
GAMMAS = [2.0, 1.4, 1.1]
NEW_SYMBOLS = ["accbpg_combine_ls_terms", "accbpg_burg_simplex_prox_acc", "accbpg_lmo_l2_ball_pos"]


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def _checksum(A):
    return np.array([A.sum(), np.abs(A).max(), (A ** 2).sum()])


def test_exports_and_signatures():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import algorithms
    E = inspect.Parameter.empty
    for name in ["AIBM", "AdaptFGM", "UniversalGM", "Poisson_regr_simplex", "Poisson_regr_simplex_acc",
                 "lmo_l2_ball_positive_orthant", "random_point_on_simplex", "edge_point_on_simplex", "get_random_float",
                 "get_random_vector"]:
        assert name in acc.__all__, name
        getattr(acc, name)
    aibm = [("f", E), ("h", E), ("L", E), ("x0", E), ("gamma", E), ("maxitrs", E), ("epsilon", 1e-14),
            ("verbose", True), ("noise", 0), ("verbskip", 1)]
    fgm = [("f", E), ("h", E), ("L", E), ("x0", E), ("maxitrs", E), ("epsilon", 1e-14), ("verbose", True),
           ("noise", 0), ("verbskip", 1)]
    ugm = fgm[:7] + [("noise_level", 0), ("verbskip", 1)]
    assert _sig(acc.AIBM) == aibm and _sig(algorithms.AIBM_steps) == aibm
    assert _sig(acc.AdaptFGM) == fgm and _sig(algorithms.AdaptFGM_steps) == fgm
    assert _sig(acc.UniversalGM) == ugm and _sig(algorithms.UniversalGM_steps) == ugm
    for fac in (acc.Poisson_regr_simplex, acc.Poisson_regr_simplex_acc):
        assert _sig(fac) == [("m", E), ("n", E), ("noise", 0.01), ("normalizeA", True)]
    assert _sig(acc.lmo_l2_ball_positive_orthant) == [("radius", E), ("center", None), ("epsilon", 0.0)]
    assert _sig(acc.random_point_on_simplex) == [("n", E), ("radius", 1), ("center", False)]
    assert _sig(acc.edge_point_on_simplex) == [("edge_index", E), ("n", E), ("radius", 1), ("tol", 1e-5)]
    assert _sig(acc.get_random_float) == [("var", 1)]
    assert _sig(acc.get_random_vector) == [("size", E), ("range", 1)]


def test_header_and_ctypes_table_carry_new_symbols():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name


def test_helpers_bit_equal_under_a_seed():
    """the package's helpers and the restatement's, against the reference's outputs and its generator state"""
    import accbpg_and_fw_amd as acc
    g = golden("inexact")
    for mod in (acc, R):
        np.random.seed(SEED)
        np.testing.assert_array_equal(mod.random_point_on_simplex(17), g["h_rand_point"])
        np.testing.assert_array_equal(mod.random_point_on_simplex(9, radius=2), g["h_rand_point_r2"])
        np.testing.assert_array_equal(mod.random_point_on_simplex(5, center=True), g["h_center_point"])
        np.testing.assert_array_equal(mod.edge_point_on_simplex(3, 8), g["h_edge_point"])
        np.testing.assert_array_equal(mod.edge_point_on_simplex(0, 6, radius=2, tol=1e-3), g["h_edge_point_r2"])
        zero = mod.get_random_float(0)
        floats = np.array([mod.get_random_float(0.5), zero, mod.get_random_float()])
        assert zero == 0 and isinstance(zero, int)
        np.testing.assert_array_equal(floats, g["h_float"])
        np.testing.assert_array_equal(mod.get_random_vector(6, 0.25), g["h_vector"])
        np.testing.assert_array_equal(mod.get_random_vector(4, 0), g["h_vector0"])
        assert np.random.random_sample() == float(g["h_after"])
        with pytest.raises(AssertionError, match="The range must be positive."):
            mod.get_random_float(-1)
        with pytest.raises(AssertionError, match="The range must be positive."):
            mod.get_random_vector(3, -1)


def test_lmo_restatement_bit_equal():
    g = golden("inexact")
    for n in (1, 2, 63, 64, 65, 1000):
        gv, c = g["lmo_g_%d" % n], g["lmo_c_%d" % n]
        np.testing.assert_array_equal(R.lmo_l2_ball_positive_orthant(1)(gv), g["lmo_s0_%d" % n])
        np.testing.assert_array_equal(R.lmo_l2_ball_positive_orthant(0.7, center=c, epsilon=1e-7)(gv), g["lmo_s1_%d" % n])
        np.testing.assert_array_equal(R.lmo_l2_ball_positive_orthant(2.0, center=c + 0.5, epsilon=0.0)(gv),
                                      g["lmo_s2_%d" % n])
        np.testing.assert_array_equal(R.lmo_l2_ball_positive_orthant(1.5, center=c - 0.5, epsilon=1e-3)(np.abs(gv)),
                                      g["lmo_pos_%d" % n])                 # early return: no assertion
    gv = np.array([-1.0, 2.0, -3.0, 0.5])
    with pytest.raises(AssertionError, match="Shape mismatch between g and center"):
        R.lmo_l2_ball_positive_orthant(1.0, center=np.zeros(3))(gv)
    with pytest.raises(AssertionError, match="Output outside L2 ball"):
        R.lmo_l2_ball_positive_orthant(1.0, epsilon=0.9)(gv)
    with pytest.raises(AssertionError, match="Output violates epsilon-nonnegativity"):
        R.lmo_l2_ball_positive_orthant(1.0, center=np.array([np.nan, 0, 0, 0]))(gv)


def test_factories_rng_sequence(monkeypatch):
    """The package's factories draw in the reference's order: A's checksum, b, L and x0 bit-equal (the objective's
    constructor, which needs a GPU, is replaced by a recorder)."""
    from accbpg_and_fw_amd import applications
    g = golden("inexact")

    class Rec:
        def __init__(self, A, b):
            self.A, self.b = A, b
    monkeypatch.setattr(applications, "PoissonRegression", Rec)
    for fac_acc, fac_fw in ((applications.Poisson_regr_simplex_acc, applications.Poisson_regr_simplex),
                            (R.Poisson_regr_simplex_acc, R.Poisson_regr_simplex)):
        np.random.seed(SEED)
        f, hs, L, x0 = fac_acc(**ACC)
        np.testing.assert_array_equal(_checksum(f.A), g["acc_A_checksum"])
        np.testing.assert_array_equal(f.b, g["acc_b"])
        np.testing.assert_array_equal(x0, g["acc_x0"])
        assert L == float(g["acc_L"]) and len(hs) == 2 and hs[0].eps == 1e-7
        np.random.seed(SEED)
        h, places = fac_fw(**FW)
        assert list(places) == list(R.PLACEMENTS) and h.eps == 1e-8
        for key, (fk, Lk, sol, x0k) in places.items():
            np.testing.assert_array_equal(_checksum(fk.A), g["fw_%s_A_checksum" % key])
            np.testing.assert_array_equal(fk.b, g["fw_%s_b" % key])
            np.testing.assert_array_equal(x0k, g["fw_%s_x0" % key])
            np.testing.assert_array_equal(sol, g["fw_%s_sol" % key])
            assert Lk == float(g["fw_%s_L" % key])


def _restated_runs(f, h, L, x0):
    runs = {}
    for ni, noise in enumerate(NOISES):
        for gamma in GAMMAS:
            runs["aibm_g%02d_n%d" % (round(gamma * 10), ni)] = \
                lambda gamma=gamma, noise=noise: R.AIBM(f, h, L, x0, gamma=gamma, maxitrs=ACC_ITERS, noise=noise)
        runs["fgm_n%d" % ni] = lambda noise=noise: R.AdaptFGM(f, h, L, x0, maxitrs=ACC_ITERS, noise=noise)
        runs["ugm_n%d" % ni] = lambda noise=noise: R.UniversalGM(f, h, L, x0, maxitrs=ACC_ITERS, noise_level=noise)
    return runs


def test_solver_restatements_reproduce_the_reference():
    """F, G, x, the L after every iteration and the lengths equal the reference's, and each call consumes the same
    number of draws from the global generator (its state after the call is the reference's)."""
    g = golden("inexact")
    np.random.seed(SEED)
    f, hs, L, x0 = R.Poisson_regr_simplex_acc(**ACC)
    for idx, (name, call) in enumerate(_restated_runs(f, hs[0], L, x0).items()):
        key = "acc_" + name
        np.random.seed(RUN_SEED + idx)
        x, F, G, Lk = call()
        assert np.random.random_sample() == float(g[key + "_after"]), name
        k0 = int(g[key + "_k0"])
        draws = int(g[key + "_draws"])
        noisy = name.endswith("n1")
        assert draws == ((len(F) if name.startswith("aibm") else len(F) - 1) if noisy else 0), (name, draws)
        np.testing.assert_array_equal(F, g[key + "_F"])
        np.testing.assert_array_equal(G, g[key + "_G"])
        np.testing.assert_array_equal(x, g[key + "_x"])
        np.testing.assert_allclose(Lk[k0:], g[key + "_Lk"], rtol=6e-4, atol=0)      # printed with four digits
        assert int(g[key + "_prefix"]) >= 60, name


def test_printed_tables_of_the_reference():
    g = golden("inexact")
    for name, title in (("aibm_g14_n0", "AIBM"), ("fgm_n0", "AdaptFGM"), ("ugm_n0", "UniversalGM")):
        head = list(g["acc_%s_head" % name])
        assert head == ["%s method for min_{x in C} F(x) = f(x) + Psi(x)" % title, "     k      F(x)       L       time"]
        assert re.fullmatch(r" {5}1 {2}[ -]\d\.\d{3}e[+-]\d\d {2} \d\.\d{3}e[+-]\d\d {2} +\d+\.\d", str(g["acc_%s_row" % name]))
