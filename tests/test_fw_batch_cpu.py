"""CPU side of the lock-step Frank-Wolfe batches: the public names, their signatures, and the four C-ABI entries in
the header and in the ctypes table.  No compute call is made."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_ENTRIES = ["accbpg_dopt_batch_fw_init", "accbpg_dopt_batch_fw_probe", "accbpg_dopt_batch_fw_update",
               "accbpg_fw_logdet_snapshot"]


def _sig(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_names_are_public():
    import accbpg_and_fw_amd as acc
    for name in ("D_opt_FW_batch", "D_opt_FW_away_batch"):
        assert name in acc.__all__ and callable(getattr(acc, name))


def test_signatures():
    import accbpg_and_fw_amd as acc
    from accbpg_and_fw_amd import D_opt_alg
    E = inspect.Parameter.empty
    plain = [("batch", E), ("x0", E), ("eps", E), ("maxitrs", E)]
    away = plain + [("logdet_refresh", None), ("logdet_ring", None)]
    assert _sig(acc.D_opt_FW_batch) == plain
    assert _sig(acc.D_opt_FW_away_batch) == away
    assert _sig(D_opt_alg.D_opt_FW_batch_steps) == plain
    assert _sig(D_opt_alg.D_opt_FW_away_batch_steps) == away
    assert inspect.isgeneratorfunction(D_opt_alg.D_opt_FW_batch_steps)
    assert inspect.isgeneratorfunction(D_opt_alg.D_opt_FW_away_batch_steps)


def test_new_entries_declared_bound_and_exported():
    from accbpg_and_fw_amd import _lib
    text = open(os.path.join(ROOT, "include", "accbpg_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(accbpg_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW_ENTRIES:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_decisions_are_shared():
    """One copy of the per-iteration decisions: the single and the lock-step solvers call the same code."""
    from accbpg_and_fw_amd import D_opt_alg
    for fn in (D_opt_alg.D_opt_FW_steps, D_opt_alg.D_opt_FW_batch_steps):
        assert "_fw_decide(" in inspect.getsource(fn)
    for fn in (D_opt_alg.D_opt_FW_away_steps, D_opt_alg.D_opt_FW_away_batch_steps):
        assert "_AwayRun(" in inspect.getsource(fn)
    eps_pos, eps_neg, upd, detmul = D_opt_alg._fw_decide(8, 8.0, 8.0, 1e-6)
    assert upd is None and eps_pos == 0.0 and eps_neg == 0.0
    eps_pos, eps_neg, upd, detmul = D_opt_alg._fw_decide(4, 6.0, 3.0, 1e-6)
    t = (6.0 / 4 - 1) / (6.0 - 1)
    assert (eps_pos, eps_neg) == (0.5, 0.25) and upd == (1 - t, t, -(t / (1 + t * 5.0)), 1 - t)


class _NumpyState:
    """The handle-side Frank-Wolfe state in NumPy, with the operations of the reference (accbpg/D_opt_alg.py:39-45,
    59-61, 76-82, 145-147): what the probe / update entries stand for, to drive the host's decision code without a GPU."""

    def __init__(self, V, x0):
        import numpy as np
        self.V, self.x = V, np.copy(x0)
        gram = np.dot(V * self.x, V.T)
        self.logdet_gram = float(np.log(np.linalg.det(gram)))
        self.H = np.linalg.inv(gram)
        self.w = np.sum(V * np.dot(self.H, V), axis=0)
        self.q = 0.0

    def probe(self, away):
        import numpy as np
        from accbpg_and_fw_amd import _lib
        w, x = self.w, self.x
        pr = _lib.FwProbe()
        i = int(np.argmax(w))
        if away:
            j = int(np.argmin((w - w[i]) * [x > 1.0e-8]))
        else:
            j = int(np.flatnonzero(x > 0)[np.argmin(w[x > 0])])
        pr.i, pr.j, pr.w_i, pr.w_j, pr.x_j, pr.q_prev = i, j, w[i], w[j], x[j], self.q
        return pr

    def update(self, p, xscale, xadd, hcoef, hdiv):
        import numpy as np
        self.x *= xscale
        self.x[p] += xadd
        Hv = np.dot(self.H, self.V[:, p])
        self.q = float(np.dot(self.V[:, p], Hv))
        self.H = (self.H + hcoef * np.outer(Hv, Hv)) / hdiv
        self.w = (self.w + hcoef * np.dot(Hv, self.V) ** 2) / hdiv


def test_decision_code_follows_the_oracle():
    """_fw_decide and _AwayRun, driven by a NumPy stand-in for the device state, walk the oracle's trajectories: gaps
    and iterates bit for bit, stopping iteration included; F of the away run identical when every iteration is
    anchored (one in flight, the last collected by the flush), within 1e-9 by the determinant lemma alone."""
    import numpy as np
    from accbpg_and_fw_amd import D_opt_alg
    from oracle import np_oracle as O
    m, n, maxitrs = 8, 40, 400
    for seed in (301, 303):
        np.random.seed(seed)
        V = np.random.randn(m, n)
        x0 = np.ones(n) / n
        # plain
        xo, Fo, SPo, SNo, _ = O.D_opt_FW(V, x0, 0.5, 80)
        st = _NumpyState(V, x0)
        det = np.exp(st.logdet_gram)
        F, SP, SN = [], [], []
        for k in range(80):
            F.append(-np.log(det))
            pr = st.probe(0)
            ep, en, upd, detmul = D_opt_alg._fw_decide(m, pr.w_i, pr.w_j, 0.5)
            SP.append(ep); SN.append(en)
            if upd is None:
                break
            st.update(pr.i, *upd)
            det *= detmul
        np.testing.assert_array_equal(SP, SPo)
        np.testing.assert_array_equal(SN, SNo)
        np.testing.assert_array_equal(st.x, xo)
        np.testing.assert_allclose(F, Fo, rtol=1e-12, atol=1e-12)
        # away: R = 1 with one anchor in flight, and R = 0
        xo, Fo, SPo, SNo, _ = O.D_opt_FW_away(V, x0, 1e-2, maxitrs)
        assert len(Fo) < maxitrs
        for R in (1, 0):
            st = _NumpyState(V, x0)
            run = D_opt_alg._AwayRun(m, maxitrs, R, 1)
            ring = []
            for k in range(maxitrs):
                collected = float("nan")
                if run.refresh(k):
                    if ring:
                        collected = ring.pop(0)
                    ring.append(float(np.log(np.linalg.det(st.H))))
                upd = run.iterate(k, st.probe(1), collected, 0.0, st.logdet_gram, 1e-2)
                if upd is None:
                    break
                st.update(*upd)
            F, SP, SN, T = run.finish(lambda: ring.pop(0))
            np.testing.assert_array_equal(SP, SPo)
            np.testing.assert_array_equal(SN, SNo)
            np.testing.assert_array_equal(st.x, xo)
            if R == 1:
                np.testing.assert_array_equal(F, Fo)
            else:
                np.testing.assert_allclose(F, Fo, rtol=1e-9, atol=1e-9)
