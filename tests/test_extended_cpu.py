"""The extended-precision fixtures (oracle/gen_extended.py, tests/golden/ext_*.npz) on the CPU: their inputs rebuild
bit for bit, the longdouble evaluation agrees with the fp64 oracle where fp64 is accurate, and the fixtures are what
they claim to be -- the row-graded ones harmless for a Cholesky-based evaluation, the nearly dependent ones a real
stress for fp64."""
import numpy as np
import pytest

from conftest import golden

from oracle import gen_extended as E
from oracle import np_oracle as O

U = 2.0 ** -53


def test_extended_evaluation_matches_fp64_when_well_conditioned():
    rs = np.random.RandomState(3)
    V = rs.randn(40, 150)
    x = rs.rand(150) + 0.1
    f, g, H = E.extended_f_g(V, x)
    fr, gr = O.DOptOracle(V).func_grad(x, 2)
    assert abs(float(f) - fr) < 1e-13 * abs(fr)
    np.testing.assert_allclose(g.astype(np.float64), gr, rtol=1e-13)
    Hr = O.DOptOracle(V).gram(x)
    np.testing.assert_allclose(H.astype(np.float64), Hr, rtol=0, atol=1e-14 * np.abs(Hr).max())


@pytest.mark.parametrize("name", sorted(E.CASES))
def test_extended_fixture_inputs_rebuild(name):
    gd = golden(name)
    kind, m, n, seed, xkind = E.CASES[name]
    V, x = E.inputs(name)
    assert V.shape == (m, n) and x.shape == (n,) and n > 2 * m
    assert E.sha(V) == str(gd["v_sha256"])
    assert E.sha(x) == str(gd["x_sha256"])
    assert gd["g"].shape == (n,) and np.all(gd["g"] < 0)
    fr, gr = O.DOptOracle(V).func_grad(x, 2)
    ef = abs(fr - float(gd["f"]))
    eg = np.max(np.abs(gr - gd["g"])) / np.max(np.abs(gd["g"]))
    if kind == "graded":
        assert ef <= 64 * m * U * abs(float(gd["f"])) and eg <= 64 * m * U, (ef, eg)
    else:
        assert float(gd["kappa"]) > 1e8
        assert eg > 64 * m * U, eg                   # fp64 loses digits here ...
        assert eg < 1e-4, eg                         # ... but the reference and the oracle still agree to kappa * u
