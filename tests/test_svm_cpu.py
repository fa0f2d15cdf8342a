"""CPU tests of the SVM family: the NumPy restatement (tests/svm_numpy.py) against the goldens the real reference wrote
(tests/golden/svm.npz, tools/gen_golden_svm.py), the closed-form PolyDiv prox against the problem the reference states,
the host-only pieces of the package (utils, the factory's arithmetic, the scalar root of the prox), and the C-ABI names.

Tolerances.  Per-call values: 1e-13 relative; a vector is held to 1e-13 of its largest entry (its entries are sums of
m terms of that size, so an entry that cancels to nearly nothing carries the rounding of the large ones).  Whole runs:
F to 1e-9 over the whole stored length and x within the reference's own spread under a 4e-16 perturbation of its
margins (0 in every stored run) + 1e-12.  KKT residual of the prox: 1e-12 relative to radius, the size of the two
terms that cancel in it."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svm_numpy as SN  # noqa: E402
from conftest import golden  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["accbpg_svm_create", "accbpg_svm_destroy", "accbpg_svm_set_stream", "accbpg_svm_func_grad",
               "accbpg_svm_get_ax"]


@pytest.fixture(scope="module")
def gold():
    return golden("svm")


def instance(tag, gold):
    if tag == "gauss":
        A, y = SN.gaussian_instance()
        np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["gauss_A_checksum"], rtol=1e-14)
        assert np.array_equal(y, gold["gauss_y"])
        return A, y
    return SN.digits_instance()


def close(a, b, rel=1e-13):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= rel * np.max(np.abs(b))), float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("tag", ["gauss", "digits"])
def test_percall_restatement_equals_goldens(gold, tag, li):
    A, y = instance(tag, gold)
    key = "pc_%s_l%d" % (tag, li)
    lamda, radius, pts = float(gold[key + "_lamda"]), float(gold[key + "_radius"]), gold[key + "_x"]
    f = SN.SVM_fun(lamda, A, y)
    h = SN.PolyDiv(A, lamda=lamda, radius=radius)
    np.testing.assert_allclose(h.DS_mean, gold[key + "_DS_mean"], rtol=1e-15)
    np.testing.assert_allclose(h.DS_mean_quad, gold[key + "_DS_mean_quad"], rtol=1e-15)
    assert float(gold[key + "_gap"]) >= 1e-6
    for i, x in enumerate(pts):
        assert np.min(np.abs(y * f.margins(x) - 1)) >= 1e-6
        np.testing.assert_allclose(f.F(x), gold[key + "_F"][i], rtol=1e-13)
        np.testing.assert_allclose(f.hinge_loss(x), gold[key + "_hinge"][i], rtol=1e-13)
        np.testing.assert_allclose(f.func_grad(x, 0), gold[key + "_f0"][i], rtol=1e-13)
        assert np.array_equal(f.indicator(x), gold[key + "_ind"][i])
        close(f.subgradient_loss(x), gold[key + "_sub"][i])
        close(f.func_grad(x, 1), gold[key + "_g1"][i])
        v, g = f.func_grad(x, 2)
        np.testing.assert_allclose(v, gold[key + "_fg_f"][i], rtol=1e-13)
        close(g, gold[key + "_fg_g"][i])
        np.testing.assert_allclose(h.h(x), gold[key + "_h"][i], rtol=1e-13)
        np.testing.assert_allclose(h(x), gold[key + "_h"][i], rtol=1e-13)
        close(h.gradient(x), gold[key + "_hgrad"][i])
        np.testing.assert_allclose(h.divergence(x, pts[(i + 1) % 3]), gold[key + "_hdiv"][i], rtol=1e-13)


def run_setup(tag, gold):
    A, y = instance(tag, gold)
    key = "run_" + tag
    lamda, L, radius, x0 = float(gold[key + "_lamda"]), float(gold[key + "_L"]), float(gold[key + "_radius"]), \
        gold[key + "_x0"]
    return A, y, lamda, L, radius, x0


RUN_NAMES = list(SN.run_table(SN.SOLVERS, SN.lmo_l2_ball))


@pytest.mark.parametrize("name", RUN_NAMES)
@pytest.mark.parametrize("tag", ["gauss", "digits"])
def test_runs_restatement_equals_goldens(gold, tag, name):
    A, y, lamda, L, radius, x0 = run_setup(tag, gold)
    f = SN.SVM_fun(lamda, A, y)
    ph, sh = SN.PolyDiv(A, lamda=lamda, radius=radius), SN.SquaredL2Norm()
    key = "run_%s_%s" % (tag, name)
    assert int(gold[key + "_prefix"]) == len(gold[key + "_F"])
    np.random.seed(SN.RUN_SEED + RUN_NAMES.index(name))
    x, F, G = SN.run_table(SN.SOLVERS, SN.lmo_l2_ball)[name](f, ph, sh, L, np.copy(x0), radius)
    assert len(F) == len(gold[key + "_F"])
    assert np.all(np.abs(F - gold[key + "_F"]) <= 1e-9 * (1 + np.abs(gold[key + "_F"])))
    assert np.max(np.abs(x - gold[key + "_x"])) <= float(gold[key + "_xspread"]) + 1e-12
    np.testing.assert_allclose(G, gold[key + "_G"], rtol=1e-9)


def test_factory_arithmetic_equals_goldens(gold):
    """the package's host-only helper and the restatement's, against the reference's factory on the digits set"""
    from accbpg_and_fw_amd.applications import _svm_ball_numbers
    X, Y = SN.digits_instance()
    for li in (0, 1):
        lamda = float(gold["fac_l%d_lamda" % li])
        for fn in (_svm_ball_numbers, SN.ball_numbers):
            np.random.seed(3)
            radius, ds_mean, ds_mean_quad, L, x0 = fn(X, Y, lamda, None)
            after = np.random.random_sample()
            assert radius == float(gold["fac_l%d_radius" % li])
            assert L == float(gold["fac_l%d_L" % li])
            assert ds_mean == float(gold["fac_l%d_DS_mean" % li])
            assert ds_mean_quad == float(gold["fac_l%d_DS_mean_quad" % li])
            assert np.array_equal(x0, gold["fac_l%d_x0" % li])
            assert after == float(gold["fac_l%d_after" % li])                   # the same draws were made
    # a centre shifts x0 and nothing else
    np.random.seed(3)
    c = np.arange(64.0)
    r2 = _svm_ball_numbers(X, Y, 0.01, c)
    assert r2[0] == float(gold["fac_l0_radius"]) and np.allclose(r2[4] - c, gold["fac_l0_x0"], rtol=0, atol=1e-12)


def test_utils_reproduce_the_reference(gold):
    from accbpg_and_fw_amd import utils as U
    for fn in (U.random_point_in_l2_ball, SN.random_point_in_l2_ball):
        np.random.seed(7)
        assert np.array_equal(fn(np.arange(9.0), 2.5), gold["u_point"])
        p = fn(np.zeros(6), 0.5, pos_dir=True)
        assert np.array_equal(p, gold["u_point_pos"]) and p.min() >= 0
        assert np.random.random_sample() == float(gold["u_after"])
    state = np.random.get_state()[1].copy()
    data, labels = U.generate_dataset_for_svm(40, 51)
    assert np.array_equal(np.random.get_state()[1], state)                      # a generator of its own
    assert data.shape == (40, 51) and labels.shape == (40,) and set(labels) <= {1, -1}
    assert 60 < data.std() < 140                                                # N(0,1) * 100
    assert [SN.svm_label(r) for r in data] == list(labels)
    assert SN.svm_label(np.r_[np.ones(52), -np.ones(48)]) == 1                  # 52 < 53
    assert SN.svm_label(np.r_[np.ones(53), -np.ones(47)]) == -1                 # 53 is not < 53


def test_abi_names_agree():
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
    for name in ("SVM_fun", "PolyDiv", "svm_digits_ds_divs_ball", "random_point_in_l2_ball", "generate_dataset_for_svm"):
        assert name in acc.__all__ and hasattr(acc, name)
    for name in ("__call__", "hinge_loss", "F", "gradient", "subgradient_loss", "func_grad", "margins"):
        assert hasattr(acc.SVM_fun, name)
    for name in ("h", "__call__", "gradient", "divergence", "extra_Psi", "prox_map", "div_prox_map", "ls_terms"):
        assert hasattr(acc.PolyDiv, name)


# ------------------------------------------------------------------------------------------- the closed-form prox
def prox_cases():
    """(name, lamda, radius, L, zero_g): t^ < radius, t^ > radius, g = 0, lamda = 0 (both sides of the radius)"""
    return [("inside", 0.5, 2.0, 5.0, False), ("boundary", 0.5, 2.0, 1e-3, False), ("zero_g", 0.5, 2.0, 1.0, True),
            ("lamda0_inside", 0.0, 2.0, 1.0, False), ("lamda0_boundary", 0.0, 2.0, 1e-3, False),
            ("big_lamda", 4.0, 0.7, 0.3, False)]


def kkt_residual(h, x, g, L):
    """|| L*phi'(t)/t * x + g' + mu*x/t || / radius with the multiplier mu = max(0, radius - L*phi'(t)) of the ball
    when x lies on its boundary and 0 inside; at x = 0 the gradient of the objective is g'"""
    gs = h.scaled(g)
    t = np.linalg.norm(x)
    if t == 0.0:
        return np.linalg.norm(gs) / h.radius, 0.0
    mu = max(0.0, h.radius - L * h.dphi(t)) if t >= h.radius * (1 - 1e-15) else 0.0
    return np.linalg.norm((L * h.dphi(t) + mu) / t * x + gs) / h.radius, mu


@pytest.mark.parametrize("case", prox_cases(), ids=lambda c: c[0])
def test_closed_form_prox(case):
    from accbpg_and_fw_amd.functions import polydiv_prox_radius
    name, lamda, radius, L, zero_g = case
    A, _ = SN.gaussian_instance()
    h = SN.PolyDiv(A, lamda=lamda, radius=radius)
    rng = np.random.RandomState(3)
    n = A.shape[1]
    g = np.zeros(n) if zero_g else rng.randn(n) * 3.0
    x = h.prox_map(g, L)
    t = np.linalg.norm(x)
    t_hat_inside = L * h.dphi(radius) > radius
    assert t <= radius * (1 + 1e-15)
    if zero_g:
        assert np.all(x == 0)
    elif name in ("inside", "lamda0_inside", "big_lamda"):
        assert t_hat_inside and t < radius * 0.999
    else:
        assert not t_hat_inside and abs(t - radius) <= 1e-15 * radius
    # the package's scalar root (safeguarded Newton) against the restatement's bisection
    tp = polydiv_prox_radius(L, lamda, h.DS_mean, h.DS_mean_quad, radius)
    assert abs(tp - h.prox_radius(L)) <= 1e-13 * radius
    if lamda == 0.0 and t_hat_inside:
        np.testing.assert_allclose(tp, radius / (L * h.DS_mean_quad), rtol=1e-14)
    # 1. KKT
    res, mu = kkt_residual(h, x, g, L)
    assert res <= 1e-12 and mu >= 0.0, (res, mu)
    # 2. no feasible point does better: 10^4 random points of the ball (uniform direction, radius^(1/n) law and
    #    a share on the boundary and along -g)
    obj = h.prox_objective(x, g, L)
    d = rng.randn(10000, n)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rho = radius * rng.rand(10000) ** (1.0 / n)
    rho[:2000] = radius
    rho[2000:4000] = radius * rng.rand(2000)
    if not zero_g:
        d[4000:5000] = -g / np.linalg.norm(g) + 0.05 * rng.randn(1000, n)
        d[4000:5000] /= np.linalg.norm(d[4000:5000], axis=1, keepdims=True)
        rho[4000:5000] = np.minimum(radius, t * (1 + 0.2 * rng.randn(1000)) + 1e-3 * rng.rand(1000))
        rho[4000:5000] = np.abs(rho[4000:5000])
    pts = d * rho[:, None]
    assert np.all(np.linalg.norm(pts, axis=1) <= radius * (1 + 1e-12))
    gs = h.scaled(g)
    vals = L * h.phi(np.linalg.norm(pts, axis=1)) + pts.dot(gs)
    slack = 1e-13 * (abs(obj) + L * h.phi(radius) + radius * radius)
    assert np.all(vals >= obj - slack), float(np.min(vals) - obj)
    # 3. ... nor a neighbour along the ray (clipped to the ball)
    if not zero_g:
        u = x / t
        for fac in (1 - 1e-6, 1 + 1e-6):
            tn = min(radius, t * fac)
            assert h.prox_objective(tn * u, g, L) >= obj - slack
    else:
        for tn in (1e-6 * radius, radius):
            assert h.prox_objective(tn * np.ones(n) / np.sqrt(n), g, L) >= obj


def test_div_prox_map_is_prox_of_shifted_gradient():
    A, _ = SN.gaussian_instance()
    h = SN.PolyDiv(A, lamda=0.5, radius=2.0)
    rng = np.random.RandomState(4)
    y, g = rng.randn(40) * 0.3, rng.randn(40)
    x = h.div_prox_map(y, g, 3.0)
    gt = g - 3.0 * h.gradient(y)
    res, mu = kkt_residual(h, x, gt, 3.0)
    assert res <= 1e-12 and mu >= 0
    assert np.isnan(h.prox_map(np.r_[np.nan, np.ones(39)], 1.0)).all()
