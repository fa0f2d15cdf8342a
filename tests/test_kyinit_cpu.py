"""CPU tests of the device Kumar-Yildirim start: its NumPy restatement (tests/ky_numpy.py, the declared summation order
with `q @ V` as the pass over V) against the oracle, and the host side of D_opt_KYinit_device (signature, the n <= 2m
branch, the legacy generator's draws, the way x0 is formed) with the device call replaced by that restatement.

The restatement sums the Gram-Schmidt dots in another order than np.dot, so it equals the oracle only where no
arg-extremum decision is within rounding of a tie.  Every instance's smallest relative top-two gap is recomputed and
held to >= 1e-9 before the comparison, so a changed instance cannot turn the comparison into a coin flip."""
import inspect
import os

import numpy as np
import pytest

import ky_numpy
from conftest import gaussian_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, n, seed of gaussian_design, np.random.seed before the start, smallest gap measured with the oracle)
INSTANCES = [(30, 1000, 4, 99, 2.6e-3), (65, 700, 6, 8, 5.3e-4), (130, 1030, 3, 11, 3.8e-6), (257, 2100, 2, 12, 2.5e-4)]


@pytest.fixture(scope="module")
def O():
    from oracle import np_oracle
    return np_oracle


@pytest.fixture(scope="module")
def cases(O):
    """per instance: V, the oracle's x0 and generator state after it, the smallest decision gap, and the restatement"""
    out = {}
    for m, n, seed, rs, _ in INSTANCES:
        V = gaussian_design(m, n, seed)
        np.random.seed(rs)
        x_ref = O.D_opt_KYinit(V)
        state = np.random.get_state()
        np.random.seed(rs)
        gap, x_gap = ky_numpy.smallest_gap(V)
        np.random.seed(rs)
        B = ky_numpy.draw_directions(m)
        picked, Q, x0 = ky_numpy.kyinit(V, B)
        for a in (V, x_ref, B, picked, Q, x0):
            a.setflags(write=False)
        out[(m, n)] = dict(V=V, x_ref=x_ref, state=state, gap=gap, x_gap=x_gap, B=B, picked=picked, Q=Q, x0=x0)
    return out


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("inst", INSTANCES, ids=lambda t: "%dx%d" % t[:2])
def test_restatement_equals_oracle(cases, inst):
    m, n, seed, rs, listed = inst
    c = cases[(m, n)]
    np.testing.assert_array_equal(c["x_gap"], c["x_ref"])       # the gap was measured on the oracle's own run
    assert c["gap"] >= 1e-9, c["gap"]
    assert 0.9 * listed <= c["gap"] <= 1.1 * listed, (c["gap"], listed)    # the instance is the one that was measured
    np.testing.assert_array_equal(c["x0"], c["x_ref"])
    Q = c["Q"]
    assert np.max(np.abs(Q.T @ Q - np.eye(m))) < 1e-12          # (unstable Gram-Schmidt, but these m are small)
    assert c["picked"].shape == (2 * m,) and c["picked"].min() >= 0 and c["picked"].max() < n


def test_restatement_equals_reference_golden(cases):
    gd = np.load(os.path.join(ROOT, "tests", "golden", "next_rows.npz"))
    c = cases[(30, 1000)]
    assert c["gap"] >= 1e-9
    np.testing.assert_array_equal(c["x0"], gd["ky_x"])


def test_tree_sums_is_the_one_block_tree():
    """tree_sums = reduce_numpy.tree_sum with one block and no final stage, at the wave and block seams"""
    from reduce_numpy import tree_sum, draw
    for m in [1, 2, 63, 64, 65, 255, 256, 257, 513, 2048]:
        t = draw(m, 3) * draw(m, 4)
        assert ky_numpy.tree_sums(t) == tree_sum(t, 1, single_block_final=False)
        rows = np.stack([t, t[::-1], 2.0 * t])
        got = ky_numpy.tree_sums(rows)
        for k in range(3):
            assert got[k] == tree_sum(rows[k], 1, single_block_final=False)


def test_deflation_differs_from_the_references_by_rounding_only():
    """the restated deflation against the oracle's recurrence (np.dot coefficients): the same subtractions in the same
    order, so only the summation order of the 17 dots separates them"""
    rng = np.random.RandomState(5)
    QT = np.linalg.qr(rng.randn(40, 40))[0].T[:17].copy()
    s = rng.randn(40)
    q = np.copy(s)
    for j in range(17):
        q = q - np.dot(QT[j], s) * QT[j]
    # either order's dot of 40 terms is within 40 eps |Q[:,j]| |s| of the exact one, so two coefficients differ by at
    # most 80 eps |s| (unit columns); each of the 17 subtractions adds a rounding of the product and of the difference
    # on either side, 4 eps |s| at most
    assert np.max(np.abs(ky_numpy.deflate(QT, s) - q)) <= 17 * (80 + 4) * np.finfo(float).eps * np.linalg.norm(s)


# ------------------------------------------------------------------ the host side of D_opt_KYinit_device
def _stub(acc, V):
    """a DOptimalObj whose device call is the NumPy restatement (no GPU here)"""
    class Stub(acc.DOptimalObj):
        def __init__(self, V):
            self.H, (self.m, self.n) = V, V.shape
            self.seen = []

        def kyinit_picks(self, B, Q_out=None):
            self.seen.append(np.array(B))
            return ky_numpy.kyinit(self.H, B)[0]
    return Stub(V)


def test_signature_and_export():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import _lib
    assert "D_opt_KYinit_device" in acc.__all__ and callable(acc.D_opt_KYinit_device)
    E = inspect.Parameter.empty
    sig = [(p.name, p.default) for p in inspect.signature(acc.D_opt_KYinit_device).parameters.values()]
    assert sig == [("V", E), ("return_picked", False)]
    assert [p.name for p in inspect.signature(acc.D_opt_KYinit).parameters.values()] == ["V"]
    assert "accbpg_dopt_kyinit" in _lib.EXPORTS and hasattr(_lib.load(), "accbpg_dopt_kyinit")
    assert hasattr(acc.DOptimalObj, "kyinit_picks")


def test_small_n_branch_leaves_the_generator_alone():
    import accbpg_and_fw_amd as acc
    np.random.seed(3)
    before = np.random.get_state()
    for m, n in [(30, 60), (30, 31), (5, 10)]:
        x0 = acc.D_opt_KYinit_device(np.zeros((m, n)))
        np.testing.assert_array_equal(x0, (1.0 / n) * np.ones(n))
        x0, picked = acc.D_opt_KYinit_device(np.zeros((m, n)), return_picked=True)
        np.testing.assert_array_equal(x0, (1.0 / n) * np.ones(n))
        assert len(picked) == 0
    assert _same_state(before, np.random.get_state())


@pytest.mark.parametrize("inst", INSTANCES[:2], ids=lambda t: "%dx%d" % t[:2])
def test_host_side_draws_and_forms_x0_as_the_reference(cases, inst):
    import accbpg_and_fw_amd as acc
    m, n, seed, rs, _ = inst
    c = cases[(m, n)]
    assert c["gap"] >= 1e-9
    f = _stub(acc, c["V"])
    np.random.seed(rs)
    x0, picked = acc.D_opt_KYinit_device(f, return_picked=True)
    assert _same_state(np.random.get_state(), c["state"])       # the generator ends where the oracle leaves it
    np.testing.assert_array_equal(f.seen[0], c["B"])            # m draws of rand(m), in step order
    np.testing.assert_array_equal(picked, c["picked"])
    np.testing.assert_array_equal(x0, c["x_ref"])
    assert abs(x0.sum() - 1.0) < 1e-15
    np.random.seed(rs)
    np.testing.assert_array_equal(acc.D_opt_KYinit_device(f), c["x_ref"])


def test_repeated_indices_are_assigned_not_accumulated():
    """accbpg/applications.py:92-94: a column picked twice gets one share, then x0 is rescaled to sum 1"""
    x0 = ky_numpy.x0_from_picked(np.array([3, 1, 3, 2]), 5)
    np.testing.assert_array_equal(x0, np.array([0, 0.25, 0.25, 0.25, 0]) / 0.75)
