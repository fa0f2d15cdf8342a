"""CPU side of the lock-step Bregman-step Frank-Wolfe batches (D_opt_FW_div_step_batch, D_opt_FW_descent_step_batch):
the public names, their signatures, the two C-ABI entries in the header and in the ctypes table, the one copy of the
per-iteration decisions, and the lock-step rules themselves -- stopping, per-instance refresh, capped trials and an
accepted capped step -- with tests/fwdiv_numpy.State standing in for the device behind a small fake batch.  Every
instance of the fake batch must come out bit for bit as fwdiv_numpy's solver run on it alone.  No GPU call is made."""
import inspect
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import fwdiv_numpy as R
from conftest import gaussian_design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["accbpg_dopt_batch_fw_div_probe", "accbpg_dopt_batch_fw_div_apply"]
FIELDS = ("i", "w_i", "x_i", "sum_w", "sum_w2", "slope", "div", "min_x", "sum_u2")


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_names_signatures_and_entries():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import D_opt_alg, _lib
    E = inspect.Parameter.empty
    R_ = D_opt_alg.REFRESH_DEFAULT
    div = [("batch", E), ("L", E), ("x0", E), ("maxitrs", E), ("gamma", E), ("epsilon", 1e-14), ("linesearch", True),
           ("ls_ratio", 2), ("radius", 1), ("refresh", R_)]
    desc = [("batch", E), ("x0", E), ("maxitrs", E), ("epsilon", 1e-14), ("radius", 1), ("refresh", R_)]
    for name in ("D_opt_FW_div_step_batch", "D_opt_FW_descent_step_batch"):
        assert name in acc.__all__ and callable(getattr(acc, name))
    assert _sig(acc.D_opt_FW_div_step_batch) == div
    assert _sig(acc.D_opt_FW_descent_step_batch) == desc
    assert _sig(D_opt_alg.D_opt_FW_div_step_batch_steps) == div
    assert _sig(D_opt_alg.D_opt_FW_descent_step_batch_steps) == desc
    assert inspect.isgeneratorfunction(D_opt_alg.D_opt_FW_div_step_batch_steps)
    assert inspect.isgeneratorfunction(D_opt_alg.D_opt_FW_descent_step_batch_steps)
    assert _sig(acc.DOptimalBatch.fw_div_probe) == [("self", E), ("active", None), ("radius", 1)]
    assert _sig(acc.DOptimalBatch.fw_div_apply) == [("self", E), ("active", E), ("applies", E)]
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name
    assert lib.accbpg_abi_version() == 3


def test_decisions_are_shared():
    """One copy of the per-iteration host logic: the sequential and the lock-step generators use the same objects, and
    the line search, the slope floor and the stop tests are written nowhere else."""
    from accbpg_and_fw_amd import D_opt_alg
    for fn in (D_opt_alg.D_opt_FW_div_step_steps, D_opt_alg.D_opt_FW_div_step_batch_steps):
        src = inspect.getsource(fn)
        assert "_DivStepRun(" in src and ".decide" in src
        assert "_step_length" not in src and "_SLOPE_FLOOR" not in src and "ls_ratio *" not in src
    for fn in (D_opt_alg.D_opt_FW_descent_step_steps, D_opt_alg.D_opt_FW_descent_step_batch_steps):
        src = inspect.getsource(fn)
        assert "_DescentRun(" in src and ".step(" in src and ".probed(" in src
        assert "sum_w2" not in src and "2 / (k + 2)" not in src


class FakeBatch:
    """What the lock-step generators ask of a DOptimalBatch, answered by one fwdiv_numpy.State per instance."""

    def __init__(self, Vs):
        self.Vs = [np.ascontiguousarray(V) for V in Vs]
        self.K = len(Vs)
        self.m, self.n = self.Vs[0].shape
        self.states = [None] * self.K
        self.recs = [None] * self.K
        self.radius = None
        self.log = []                                           # (call, instances it covered)

    def _idx(self, active):
        return [i for i in range(self.K) if active is None or active[i]]

    def fw_rows(self, x0):
        x0 = np.asarray(x0, dtype=np.float64)
        X = np.tile(x0, (self.K, 1)) if x0.ndim == 1 else x0.copy()
        assert X.shape == (self.K, self.n)
        return X, True

    def fw_init(self, X, active=None, named=False):
        idx = self._idx(active)
        self.log.append(("init", tuple(idx)))
        out = [float("nan")] * self.K
        for i in idx:
            try:
                if self.states[i] is None:
                    self.states[i] = R.State(self.Vs[i], X[i])
                else:
                    self.states[i].init(np.array(X[i], dtype=np.float64))
            except ValueError as err:
                raise ValueError(("instance %d: " % i if named else "") + str(err)) from None
            self.recs[i] = None
            out[i] = self.states[i].ld
        return out

    def fw_x(self, i, as_numpy=True):
        return self.states[i].x.copy()

    def fw_div_probe(self, active=None, radius=1):
        idx = self._idx(active)
        self.log.append(("probe", tuple(idx)))
        self.radius = radius
        out = [None] * self.K
        for i in idx:
            self.recs[i] = self.states[i].probe(radius)
            out[i] = SimpleNamespace(**{k: self.recs[i][k] for k in FIELDS})
        return out

    def fw_div_apply(self, active, applies):
        idx = self._idx(active)
        self.log.append(("apply", tuple(idx)))
        for i in idx:
            p, a, hcoef, hdiv = applies[i]
            assert self.recs[i] is not None and p == self.recs[i]["i"], "apply without the probe before it"
            self.states[i].apply(self.recs[i], a, self.radius, hcoef, hdiv)
            self.recs[i] = None

    def fw_div_capped(self, i, p, radius, valued):
        self.log.append(("capped", (i,)))
        st = self.states[i]
        s = np.full(self.n, R.FILL)
        s[p] = radius
        trial = st.x + 1.0 * (s - st.x)
        return trial, (R._value(st.V, trial) if valued else None)


def _same(got, want, what):
    np.testing.assert_array_equal(got, want, err_msg=what)


def test_staggered_stops():
    from accbpg_and_fw_amd import D_opt_alg
    m, n, maxitrs = 8, 40, 400
    Vs = [gaussian_design(m, n, seed) for seed in range(301, 306)]
    x0 = np.ones(n) / n
    fake = FakeBatch(Vs)
    out = D_opt_alg.D_opt_FW_div_step_batch(fake, 1.0, x0, maxitrs, 2.0, epsilon=1e-3)
    lens = [len(F) for _, F, _, _ in out]
    print("div step lengths", lens)
    assert lens == [184, 159, 165, 182, 185]
    assert len(set(lens)) == len(lens) and max(lens) < maxitrs
    for i, (x, F, Ls, T) in enumerate(out):
        xr, Fr, Lsr = R.fw_div_step(Vs[i], 1.0, x0, maxitrs, 2.0, epsilon=1e-3)
        _same(x, xr, "x %d" % i); _same(F, Fr, "F %d" % i); _same(Ls, Lsr, "Ls %d" % i)
        assert len(T) == len(F)
    # an instance that has stopped takes part in no later launch
    probes = [idx for call, idx in fake.log if call == "probe"]
    assert len(probes) == max(lens)
    for k, idx in enumerate(probes):
        assert idx == tuple(i for i in range(5) if lens[i] > k), k

    fake = FakeBatch(Vs)
    out = D_opt_alg.D_opt_FW_descent_step_batch(fake, x0, maxitrs, epsilon=1e-3)
    lens = [len(F) for _, F, _, _ in out]
    print("descent lengths", lens)
    assert lens == [23, 56, 28, 48, 36]
    assert len(set(lens)) == len(lens) and max(lens) < maxitrs
    for i, (x, F, T, G) in enumerate(out):
        xr, Fr = R.fw_descent_step(Vs[i], x0, maxitrs, epsilon=1e-3)
        _same(x, xr, "x %d" % i); _same(F, Fr, "F %d" % i)
        assert len(T) == len(G) == len(F) and not G.any()
    probes = [idx for call, idx in fake.log if call == "probe"]
    assert len(probes) == max(lens)
    for k, idx in enumerate(probes):
        assert idx == tuple(i for i in range(5) if lens[i] > k), k


def _capped_batch():
    V = gaussian_design(16, 257, 2)
    return [V, V, V], np.ones(257) / 257, [1.0, 1e-9, 1.0]


def test_capped_trials_with_the_line_search():
    """Instance 1 starts from a tiny L: its first trials sit at the cap and are valued in full on its own, its
    neighbours share every launch all the same."""
    from accbpg_and_fw_amd import D_opt_alg
    Vs, x0, L = _capped_batch()
    fake = FakeBatch(Vs)
    out = D_opt_alg.D_opt_FW_div_step_batch(fake, L, x0, 12, 2.0)
    for i, (x, F, Ls, T) in enumerate(out):
        xr, Fr, Lsr = R.fw_div_step(Vs[i], L[i], x0, 12, 2.0)
        _same(x, xr, "x %d" % i); _same(F, Fr, "F %d" % i); _same(Ls, Lsr, "Ls %d" % i)
    assert out[1][2][0] == 0.067108864
    capped = [idx for call, idx in fake.log if call == "capped"]
    assert capped and set(capped) == {(1,)}
    assert all(idx == (0, 1, 2) for call, idx in fake.log if call in ("probe", "apply"))
    assert [idx for call, idx in fake.log if call == "init"] == [(0, 1, 2)]      # every capped trial was rejected


def test_accepted_capped_step_reinitialises_that_instance_alone():
    from accbpg_and_fw_amd import D_opt_alg
    Vs, x0, L = _capped_batch()
    fake = FakeBatch(Vs)
    out = D_opt_alg.D_opt_FW_div_step_batch(fake, L, x0, 12, 2.0, linesearch=False, refresh=5)
    for i, (x, F, Ls, T) in enumerate(out):
        xr, Fr, Lsr = R.fw_div_step(Vs[i], L[i], x0, 12, 2.0, linesearch=False, refresh=5)
        _same(x, xr, "x %d" % i); _same(F, Fr, "F %d" % i); _same(Ls, Lsr, "Ls %d" % i)
    F1 = out[1][1]
    print("instance 1 F", F1[:3])
    assert abs(F1[0] - 0.121) < 1e-3 and abs(F1[1] - 431.4) < 0.1
    # L stays tiny without the line search: instance 1 sits at the cap in every iteration, so each of its steps is a
    # re-initialisation of it alone and it takes part in no batched apply; its `since` never reaches the refresh that
    # its neighbours take together after 5 and 10 steps
    inits = [idx for call, idx in fake.log if call == "init"]
    assert inits[0] == (0, 1, 2) and inits[1] == (1,)
    assert inits.count((1,)) == 12 and inits.count((0, 2)) == 2 and len(inits) == 15
    assert [idx for call, idx in fake.log if call == "apply"] == [(0, 2)] * 12
    assert [idx for call, idx in fake.log if call == "probe"] == [(0, 1, 2)] * 12
    k5 = [j for j, e in enumerate(fake.log) if e == ("init", (0, 2))][0]
    assert sum(1 for c, _ in fake.log[:k5] if c == "probe") == 5 and fake.log[k5 + 1][0] == "probe"


def test_exceptions_name_the_instance():
    from accbpg_and_fw_amd import D_opt_alg
    Vs, x0, L = _capped_batch()

    class Rising(FakeBatch):
        def fw_div_probe(self, active=None, radius=1):
            out = super().fw_div_probe(active, radius)
            out[2].slope = 1.0
            return out
    with pytest.raises(ValueError, match=r"^instance 2: grad_d_prod must be non-positive$"):
        D_opt_alg.D_opt_FW_div_step_batch(Rising(Vs), 1.0, x0, 3, 2.0)

    class Zero(FakeBatch):
        def fw_div_probe(self, active=None, radius=1):
            out = super().fw_div_probe(active, radius)
            out[1].min_x = 0.0
            return out
    with pytest.raises(AssertionError, match=r"^instance 1: Entries of x or y not positive\.$"):
        D_opt_alg.D_opt_FW_div_step_batch(Zero(Vs), 1.0, x0, 3, 2.0)

    # a vertex is singular for m > 1 once the floor vanishes: the re-initialisation of the capped step raises, named
    class Singular(FakeBatch):
        def fw_init(self, X, active=None, named=False):
            if active is not None and list(active) == [False, True, False]:
                X = X.copy()
                X[1] = np.where(X[1] > 0.5, X[1], 0.0)
            return super().fw_init(X, active, named)
    with pytest.raises(ValueError, match=r"^instance 1: HXHT is singular or not positive definite$"):
        D_opt_alg.D_opt_FW_div_step_batch(Singular(Vs), L, x0, 3, 2.0, linesearch=False)
    with pytest.raises(ValueError, match=r"^instance 0: Initial L must be positive$"):
        D_opt_alg.D_opt_FW_div_step_batch(FakeBatch(Vs), [0.0, 1.0, 1.0], x0, 3, 2.0)
