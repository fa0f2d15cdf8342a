"""CPU tests of the Bregman-step Frank-Wolfe solvers on the maintained state: the public names and signatures, the
C-ABI record, and the NumPy restatement (tests/fwdiv_numpy.py: the rank-one arithmetic of DESIGN.md 6f in float64)
against the real reference's traces under tests/golden and against the NumPy oracle.

Bars.  Bregman step: Ls equal to 1e-12 over the whole run, F within 1e-11 relative to max(1, |F|) (the bar of
tests/test_oracle.py for this solver), x within 1e-11; with refresh 256, 0 and 64.  Classical step with refresh 256:
F within 1e-9, x within 1e-11."""
import inspect
import os
import re

import numpy as np
import pytest

import fwdiv_numpy as R
from oracle import np_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOUSING = os.path.join(ROOT, "tests", "golden", "data", "housing.txt")


@pytest.fixture(scope="module")
def gold():
    out = dict(np.load(os.path.join(ROOT, "tests", "golden", "fwdiv.npz")))
    nr = np.load(os.path.join(ROOT, "tests", "golden", "next_rows.npz"))
    for k in nr.files:
        if "_fwdiv_" in k:
            out[k] = nr[k]
    return out


@pytest.fixture(scope="module")
def instances():
    return {"h": O.D_opt_libsvm(HOUSING), "r": O.D_opt_design(80, 200, randseed=10),
            "s": O.D_opt_design(64, 512, randseed=3)}


def test_public_names_and_signatures():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import D_opt_alg
    E = inspect.Parameter.empty

    def sig(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]
    div = [("f", E), ("L", E), ("x0", E), ("maxitrs", E), ("gamma", E), ("epsilon", 1e-14), ("linesearch", True),
           ("ls_ratio", 2), ("verbose", True), ("verbskip", 1), ("radius", 1), ("refresh", 256)]
    desc = [("f", E), ("x0", E), ("maxitrs", E), ("epsilon", 1e-14), ("verbose", True), ("verbskip", 1), ("radius", 1),
            ("refresh", 256)]
    assert sig(acc.D_opt_FW_div_step) == sig(D_opt_alg.D_opt_FW_div_step_steps) == div
    assert sig(acc.D_opt_FW_descent_step) == sig(D_opt_alg.D_opt_FW_descent_step_steps) == desc
    for name in ("D_opt_FW_div_step", "D_opt_FW_descent_step"):
        assert name in acc.__all__ and callable(getattr(acc, name))
    # the generic solvers keep their signatures and point to the specialised ones
    generic = sig(acc.FW_alg_div_step)
    assert [n for n, _ in generic] == ["f", "h", "L", "x0", "maxitrs", "gamma", "lmo", "epsilon", "linesearch",
                                       "ls_ratio", "verbose", "verbskip"]
    assert "D_opt_FW_div_step" in acc.FW_alg_div_step.__doc__
    assert "D_opt_FW_descent_step" in acc.FW_alg_descent_step.__doc__


def test_option_checks_come_before_any_device_work():
    import accbpg_and_fw_amd as acc
    for kwargs, msg in ((dict(L=1.0, ls_ratio=0.5), "ls_ratio must be >= 1"), (dict(L=0.0), "Initial L must be positive"),
                        (dict(L=1.0, epsilon=0.0), "epsilon must be positive")):
        with pytest.raises(ValueError, match=msg):
            acc.D_opt_FW_div_step(None, x0=None, maxitrs=3, gamma=2.0, verbose=False, **kwargs)


def test_record_layout_matches_the_header():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    body = re.search(r"typedef struct accbpg_fw_div_probe \{(.*?)\} accbpg_fw_div_probe;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            kind, rest = decl.split(None, 1)
            names += [(n.strip(), kind) for n in rest.split(",")]
    assert [n for n, _ in names] == [n for n, _ in _lib.FwDivProbe._fields_]
    assert names[0][1] == "int64_t" and all(k == "double" for _, k in names[1:])
    import ctypes
    assert ctypes.sizeof(_lib.FwDivProbe) == 8 * len(names)
    lib = _lib.load()
    assert hasattr(lib, "accbpg_fw_div_probe_step") and hasattr(lib, "accbpg_fw_div_apply")


def _dev(F, Fr):
    return float(np.max(np.abs(F - Fr) / np.maximum(1, np.abs(Fr))))


def _check_div(got, gold, tag, what):
    x, F, Ls = got
    assert len(F) == len(gold[tag + "_F"]) == len(Ls)
    dl, df, dx = float(np.max(np.abs(Ls - gold[tag + "_Ls"]))), _dev(F, gold[tag + "_F"]), \
        float(np.max(np.abs(x - gold[tag + "_x"])))
    print("%-22s Ls %.1e  F %.2e  x %.2e" % (what, dl, df, dx))
    assert dl <= 1e-12 and df <= 1e-11 and dx <= 1e-11, (what, dl, df, dx)


@pytest.mark.parametrize("refresh", [256, 0, 64])
def test_div_step_restatement_against_the_reference(gold, instances, refresh):
    for tag in ("h", "r"):
        f, h, L, x0 = instances[tag]
        _check_div(R.fw_div_step(f.H, L, x0, 300, 2.0, ls_ratio=2, refresh=refresh), gold, tag + "_fwdiv",
                   "%s refresh %d" % (tag, refresh))
    f, h, L, x0 = instances["s"]
    assert L == float(gold["s_L"])
    _check_div(R.fw_div_step(f.H, L, x0, 600, 2.0, ls_ratio=1.5, refresh=refresh), gold, "s_ls15",
               "s ls 1.5 refresh %d" % refresh)
    _check_div(R.fw_div_step(f.H, L, x0, 600, 2.0, linesearch=False, refresh=refresh), gold, "s_nols",
               "s no ls refresh %d" % refresh)


def test_descent_step_restatement_against_the_reference(gold, instances):
    for tag in ("h", "r"):
        f, h, L, x0 = instances[tag]
        x, F = R.fw_descent_step(f.H, x0, 600, refresh=256)
        assert len(F) == len(gold[tag + "_desc_F"])
        df, dx = _dev(F, gold[tag + "_desc_F"]), float(np.max(np.abs(x - gold[tag + "_desc_x"])))
        print("descent %s  F %.2e  x %.2e" % (tag, df, dx))
        assert df <= 1e-9 and dx <= 1e-11


def test_div_step_restatement_against_the_oracle():
    f, h, L, x0 = O.D_opt_design(30, 1000, randseed=4)
    xo, Fo, Lso, _ = O.FW_alg_div_step(f, h, L, x0, 400, 2.0, O.lmo_simplex(), verbose=False)
    x, F, Ls = R.fw_div_step(f.H, L, x0, 400, 2.0)
    assert len(F) == len(Fo)
    assert np.max(np.abs(Ls - Lso)) <= 1e-12 and _dev(F, Fo) <= 1e-11 and np.max(np.abs(x - xo)) <= 1e-11


def test_floor_term_is_needed_and_bounded():
    """Without the first-order term q * sum w the value is off by q * sum w; with it the value meets 1e-12.  The bound:
    V X V^T >= min(x) V V^T, so sum w = tr(H V V^T) <= m / min(x) (= m n at the uniform start) and q <= fill."""
    f, h, L, x0 = O.D_opt_design(64, 512, randseed=3)
    st = R.State(f.H, x0)
    for _ in range(20):
        rec = st.probe(1)
        hcoef, hdiv, ld1, q1, f1 = R.step_scalars(0.2, 1, rec, st.ld, st.q, st.m)
        st.apply(rec, 0.2, 1, hcoef, hdiv)
        st.ld, st.q = ld1, q1
    rec = st.probe(1)
    exact = R._value(st.V, st.x)
    with_term, without = -st.ld - st.q * rec["sum_w"], -st.ld
    assert 0 < st.q <= R.FILL
    assert abs(with_term - exact) <= 1e-12 * abs(exact) < abs(without - exact)
    assert st.q * rec["sum_w"] <= R.FILL * st.m / st.x.min()
    # the trial value predicted for a step is the value at the point reached
    hcoef, hdiv, ld1, q1, f1 = R.step_scalars(0.3, 1, rec, st.ld, st.q, st.m)
    st.apply(rec, 0.3, 1, hcoef, hdiv)
    assert abs(f1 - R._value(st.V, st.x)) <= 1e-12 * abs(f1)
