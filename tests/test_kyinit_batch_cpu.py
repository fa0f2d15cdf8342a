"""CPU side of the batched Kumar-Yildirim start (D_opt_KYinit_batch, accbpg_dopt_batch_kyinit): the public name and its
signature, the C-ABI entry in the header and in the ctypes table, the n <= 2m branch (no GPU, generator untouched), the
host side (draw order, the way the rows of x0 are formed) with the device call replaced by the NumPy restatement
tests/ky_numpy.py, and the decision gaps of the instance sets that tests/test_gpu_kyinit_batch.py compares with the host
D_opt_KYinit.

That comparison holds only where no arg-extremum decision is within rounding of a tie, so every instance's
smallest relative top-two gap is recomputed here with the oracle's recurrences and held to >= 1e-9, and to the figure
that was measured when the sets were chosen."""
import inspect
import os
import re

import numpy as np
import pytest

import ky_numpy
from conftest import gaussian_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (m, n, seeds of gaussian_design, np.random.seed before the starts, smallest gap of each instance measured with the
# oracle's recurrences, the generator running on from one instance to the next)
SETS = [(30, 1000, (4, 5, 6), 99, (2.6e-3, 1.9e-4, 9.6e-4)),
        (65, 700, (6, 7, 8, 9), 8, (5.3e-4, 8.8e-4, 1.2e-4, 1.2e-3)),
        (130, 1030, (3, 4), 11, (3.8e-6, 5.5e-4))]


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_signature_and_export():
    import accbpg_and_fw_amd as acc
    assert "D_opt_KYinit_batch" in acc.__all__ and callable(acc.D_opt_KYinit_batch)
    E = inspect.Parameter.empty
    sig = [(p.name, p.default) for p in inspect.signature(acc.D_opt_KYinit_batch).parameters.values()]
    assert sig == [("batch", E), ("return_picked", False)]
    sig = [(p.name, p.default) for p in inspect.signature(acc.DOptimalBatch.kyinit_picks).parameters.values()]
    assert sig == [("self", E), ("B", E), ("Q_out", None)]


def test_entry_declared_bound_and_exported():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+accbpg_dopt_batch_kyinit\s*\(([^)]*)\)\s*;", text)
    assert decl, "accbpg_dopt_batch_kyinit is not declared"
    args = [" ".join(a.split()) for a in decl.group(1).split(",")]
    assert args == ["accbpg_dopt_batch* b", "const double* B_dev", "int64_t* picked_host", "double* Q_dev"]
    assert "accbpg_dopt_batch_kyinit" in _lib.EXPORTS
    lib = _lib.load()
    assert hasattr(lib, "accbpg_dopt_batch_kyinit")
    assert lib.accbpg_dopt_batch_kyinit.argtypes == lib.accbpg_dopt_kyinit.argtypes     # (handle, B, picked, Q)


def test_small_n_branch_needs_no_gpu_and_leaves_the_generator_alone():
    import accbpg_and_fw_amd as acc
    np.random.seed(3)
    before = np.random.get_state()
    Vs = [np.zeros((30, 60)) for _ in range(3)]
    X0 = acc.D_opt_KYinit_batch(Vs)
    assert X0.shape == (3, 60)
    np.testing.assert_array_equal(X0, (1.0 / 60) * np.ones((3, 60)))
    X0, picked = acc.D_opt_KYinit_batch(Vs, return_picked=True)
    np.testing.assert_array_equal(X0, (1.0 / 60) * np.ones((3, 60)))
    assert picked.shape == (3, 0) and picked.dtype == np.int64
    assert _same_state(before, np.random.get_state())


@pytest.fixture(scope="module")
def sets():
    """per set: the matrices (built first: gaussian_design reseeds the generator), then under np.random.seed(rs) the
    oracle's gap and start of instance after instance, and the generator state at the end"""
    out = {}
    for m, n, seeds, rs, _ in SETS:
        Vs = [gaussian_design(m, n, seed) for seed in seeds]
        np.random.seed(rs)
        runs = [ky_numpy.smallest_gap(V) for V in Vs]
        state = np.random.get_state()
        for V in Vs:
            V.setflags(write=False)
        out[(m, n)] = dict(Vs=Vs, gaps=[g for g, _ in runs], x_ref=np.stack([x for _, x in runs]), state=state)
    return out


@pytest.mark.parametrize("case", SETS, ids=lambda t: "%dx%dx%d" % (t[0], t[1], len(t[2])))
def test_end_to_end_instances_are_free_of_near_ties(sets, case):
    m, n, seeds, rs, listed = case
    gaps = sets[(m, n)]["gaps"]
    for gap, want in zip(gaps, listed):
        assert gap >= 1e-9, gaps
        assert 0.9 * want <= gap <= 1.1 * want, (gaps, listed)  # the instance is the one that was measured


def _stub_batch(acc, Vs):
    """a DOptimalBatch whose device call is the NumPy restatement (no GPU here)"""
    class Stub(acc.DOptimalBatch):
        def __init__(self, Vs):
            self.Vs, self.K, (self.m, self.n) = Vs, len(Vs), Vs[0].shape
            self.seen = []

        def kyinit_picks(self, B, Q_out=None):
            self.seen.append(np.array(B))
            return np.stack([ky_numpy.kyinit(V, Bi)[0] for V, Bi in zip(self.Vs, B)])
    return Stub(Vs)


@pytest.mark.parametrize("case", SETS[:2], ids=lambda t: "%dx%dx%d" % (t[0], t[1], len(t[2])))
def test_host_side_draws_instance_by_instance_and_forms_the_rows_as_the_reference(sets, case):
    import accbpg_and_fw_amd as acc
    m, n, seeds, rs, _ = case
    c = sets[(m, n)]
    assert min(c["gaps"]) >= 1e-9
    batch = _stub_batch(acc, c["Vs"])
    np.random.seed(rs)
    X0, picked = acc.D_opt_KYinit_batch(batch, return_picked=True)
    assert _same_state(np.random.get_state(), c["state"])       # the generator ends where the loop of starts leaves it
    np.random.seed(rs)
    B = np.stack([ky_numpy.draw_directions(m) for _ in seeds])
    np.testing.assert_array_equal(batch.seen[0], B)             # m draws of rand(m) per instance, in step order
    assert X0.shape == (len(seeds), n) and picked.shape == (len(seeds), 2 * m) and picked.dtype == np.int64
    np.testing.assert_array_equal(X0, c["x_ref"])
    for i in range(len(seeds)):
        np.testing.assert_array_equal(X0[i], ky_numpy.x0_from_picked(picked[i], n))
    np.random.seed(rs)
    np.testing.assert_array_equal(acc.D_opt_KYinit_batch(batch), c["x_ref"])
