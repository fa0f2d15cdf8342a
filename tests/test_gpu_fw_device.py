"""``accbpg_fw_run`` and the solvers built on it (D_opt_FW_device, D_opt_FW_away_device): several iterations per host
round trip, the scalar decisions taken on the device.

The bar throughout is EQUALITY with the step-by-step path on the same data -- ``accbpg_fw_probe_step`` /
``accbpg_fw_update`` with the host's decisions, or the sequential solvers -- for x, F, SP, SN, the iteration count, the
records and the state (x, w, H): the run kernels wrap the same bodies on the same grids, and the decisions are correctly
rounded float64 + - * / written in the same order, so there is nothing to tolerate.  On axis designs the NumPy
restatement (tests/fw_numpy.py) is matched bit for bit as well."""
import ctypes as C

import numpy as np
import pytest

import fw_numpy as N
from conftest import gaussian_design, golden
from test_gpu_fw_steps import Dev, _shape, _shape_support

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

INF, NAN = float("inf"), float("nan")
APPLIED, STOPPED, BAD_PIVOT, NOT_RUN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def L(acc):
    from accbpg_and_fw_amd import _lib
    return _lib


def _same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b, err_msg=str(what))


def _obj_state(L, obj):
    m, n = obj.m, obj.n
    x = torch.empty(n, dtype=torch.float64, device="cuda")
    w = torch.empty(n, dtype=torch.float64, device="cuda")
    H = torch.empty(m, m, dtype=torch.float64, device="cuda")
    assert L.load().accbpg_fw_get_state(obj._h, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                        C.c_void_p(H.data_ptr())) == L.OK
    return x.cpu().numpy(), w.cpu().numpy(), H.cpu().numpy()


# ------------------------------------------------------------------------------- the two paths through the C-ABI
FIELDS = ("i", "j", "w_i", "w_j", "x_j", "q_prev", "p", "xscale", "xadd", "hcoef", "hdiv", "kind", "status")


def run_chunk(L, dev, away, eps, nsteps):
    """accbpg_fw_run: (rc, nrun, every record as a tuple in FIELDS order)"""
    steps = (L.FwStep * nsteps)()
    nrun = C.c_int(-1)
    rc = dev.lib.accbpg_fw_run(dev.h, int(away), float(eps), int(nsteps), steps, C.byref(nrun))
    return rc, nrun.value, [tuple(getattr(s, f) for f in FIELDS) for s in steps]


class Sequential:
    """The same iterations one at a time: probe, the package's own decision code on the host, update."""

    def __init__(self, L, dev, away):
        from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
        self.L, self.dev, self.away, self.k = L, dev, away, 0
        self.decide = _fw_decide
        self.arun = _AwayRun(dev.m, 4096, 0, 1)

    def steps(self, eps, nsteps):
        """records as run_chunk returns them (status 3 behind a stop), and the update's return code"""
        out, rc = [], self.L.OK
        for _ in range(nsteps):
            if out and out[-1][-1] != APPLIED:
                out.append((0, 0, 0.0, 0.0, 0.0, 0.0, -1, 0.0, 0.0, 0.0, 0.0, -1, NOT_RUN))
                continue
            pr = self.dev.probe(self.away)
            if self.away:
                upd = self.arun.iterate(self.k, pr, NAN, 0.0, 0.0, eps)
            else:
                u = self.decide(self.dev.m, pr.w_i, pr.w_j, eps)[2]
                upd = None if u is None else (pr.i,) + u
            head = (pr.i, pr.j, pr.w_i, pr.w_j, pr.x_j, pr.q_prev)
            if upd is None:
                out.append(head + (-1, 0.0, 0.0, 0.0, 0.0, -1, STOPPED))
                continue
            kind = 0 if not (self.away and not self.arun.SP[self.k] >= self.arun.SN[self.k]) else 1
            rc = self.dev.lib.accbpg_fw_update(self.dev.h, int(upd[0]), *[float(v) for v in upd[1:]])
            status = APPLIED if rc == self.L.OK else BAD_PIVOT
            out.append(head + tuple(upd) + (kind, status))
            self.k += 1
        return rc, out


def _records_equal(got, want, what):
    """every field (NaN equals NaN)"""
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for f, a, b in zip(FIELDS, g, w):
            np.testing.assert_array_equal(a, b, err_msg="%s: record %d field %s" % (what, k, f))


def _two(L, V, x0, ldv=None, prepare=None):
    a, b = Dev(L, V, ldv), Dev(L, V, ldv)
    for d in (a, b):
        d.init(x0)
        if prepare is not None:
            prepare(d)
    return a, b


def _both_paths(L, V, x0, away, eps, chunks, ldv=None, prepare=None, what=""):
    """``chunks`` of iterations by accbpg_fw_run on one handle and one at a time on another: equal records, equal
    return codes, equal state after every chunk."""
    a, b = _two(L, V, x0, ldv, prepare)
    with a, b:
        seq = Sequential(L, b, away)
        for c, nsteps in enumerate(chunks):
            rc, nrun, recs = run_chunk(L, a, away, eps, nsteps)
            rc_s, want = seq.steps(eps, nsteps)
            assert rc == rc_s, (what, c, rc, rc_s, L.last_error())
            assert nrun == sum(1 for r in want if r[-1] != NOT_RUN)
            _records_equal(recs, want, (what, c))
            _same(a.state(), b.state(), (what, c))
            if recs[nrun - 1][-1] != APPLIED:
                return recs
    return recs


# ---------------------------------------------------------------------------------- the notebook shape, chunk sizes
@pytest.fixture(scope="module")
def notebook(acc):
    V = gaussian_design(30, 1000, 10)
    x0 = np.ones(1000) / 1000
    obj = acc.DOptimalObj(V)
    fw = acc.D_opt_FW(obj, x0, 1e-9, 300, verbose=False)
    away = acc.D_opt_FW_away(obj, x0, 1e-9, 300, verbose=False)
    assert len(fw[1]) == 300 and len(away[1]) == 300
    return obj, x0, fw, away


@pytest.mark.parametrize("S", [1, 2, 7, 64])
def test_chunk_sizes_at_the_notebook_shape(acc, notebook, S):
    """(30, 1000) seed 10, 300 iterations: chunk sizes that do and do not divide maxitrs (and, for the away variant,
    the 16 iterations between two anchors)."""
    obj, x0, fw, away = notebook
    got = acc.D_opt_FW_device(obj, x0, 1e-9, 300, verbose=False, sync_every=S)
    _same(got[:4], fw[:4], "FW")
    assert np.all(np.diff(got[4]) >= 0) and len(set(got[4])) <= (300 + S - 1) // S
    got = acc.D_opt_FW_away_device(obj, x0, 1e-9, 300, verbose=False, sync_every=S)
    _same(got[:4], away[:4], "away")
    got = acc.D_opt_FW_away_device(obj, x0, 1e-9, 300, verbose=False, sync_every=S, logdet_refresh=0)
    _same(got[:4], acc.D_opt_FW_away(obj, x0, 1e-9, 300, verbose=False, logdet_refresh=0)[:4], "away, R = 0")


def test_notebook_shape_follows_the_stored_trace(acc):
    """S = 64 against tests/golden/fw_30x1000.npz at the bars of test_gpu_parity.test_fw_trajectories"""
    gd = golden("fw_30x1000")
    m, n, seed, iters = int(gd["m"]), int(gd["n"]), int(gd["seed"]), int(gd["iters"])
    V = gaussian_design(m, n, seed)
    x0 = np.ones(n) / n
    x, F, SP, SN, T = acc.D_opt_FW_device(V, x0, float(gd["eps"]), iters, verbose=False, sync_every=64)
    assert len(F) == len(gd["fw_F"])
    assert np.max(np.abs(x - gd["fw_x"])) < 1e-9
    for a, b in ((F, gd["fw_F"]), (SP, gd["fw_SP"]), (SN, gd["fw_SN"])):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9)
    x, F, SP, SN, T = acc.D_opt_FW_away_device(V, x0, float(gd["eps"]), iters, verbose=False, sync_every=64)
    assert abs(len(F) - len(gd["away_F"])) <= 2
    k = min(len(F), len(gd["away_F"]))
    assert np.max(np.abs(x - gd["away_x"])) < 1e-8
    np.testing.assert_allclose(F[:k], gd["away_F"][:k], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(SP[:k], gd["away_SP"][:k], rtol=1e-8, atol=1e-8)


@pytest.mark.parametrize("R", [16, 5, 1, 0])
def test_away_chunks_are_cut_at_the_anchors(acc, R):
    """(64, 512): F[k] = log det(H_k), anchored every R-th iteration, is compared as well"""
    V = gaussian_design(64, 512, 19)
    x0 = np.ones(512) / 512
    obj = acc.DOptimalObj(V)
    want = acc.D_opt_FW_away(obj, x0, 1e-9, 100, verbose=False, logdet_refresh=R)
    assert len(want[1]) == 100
    for S in (None, 7):
        got = acc.D_opt_FW_away_device(obj, x0, 1e-9, 100, verbose=False, sync_every=S, logdet_refresh=R)
        _same(got[:4], want[:4], (R, S))
    if R == 1:
        got = acc.D_opt_FW_away_device(obj, x0, 1e-9, 100, verbose=False, logdet_refresh=1, logdet_ring=1)
        _same(got[:4], acc.D_opt_FW_away(obj, x0, 1e-9, 100, verbose=False, logdet_refresh=1, logdet_ring=1)[:4])


# -------------------------------------------------------------------------------------- stops, bit for bit
def _stop_eps(SP, SN):
    """(k, eps): the stop test first holds at k = 3 mod 7"""
    gap = np.maximum(SP, SN)
    for k in range(3, len(gap), 7):
        if np.all(gap[:k] > gap[k]):
            return k, float(gap[k])
    raise AssertionError("no iteration k = 3 mod 7 at which the gap is a strict running minimum")


@pytest.mark.parametrize("m,n,start", N.RUN_SHAPES)
@pytest.mark.parametrize("away", [0, 1])
def test_stop_in_mid_chunk_and_at_the_start(acc, L, m, n, start, away):
    """Axis designs: the sequential solver, the device form with S = 7 and the NumPy restatement stop at the same
    k = 3 mod 7 with the same x, SP, SN -- and the same (x, w, H): the kernels behind the stop changed nothing.  Then
    eps so large that the start already meets the stop test."""
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    s, x0 = N.axis_run_design(m, n, start)
    V, G = N.axis_design(m, n, s, x0)
    make_run = lambda m_, it: _AwayRun(m_, it, 0, 1)
    chain = (lambda eps: N.run_away(V, x0, eps, 60, make_run)) if away else (lambda eps: N.run_fw(V, x0, eps, 60, _fw_decide))
    free = chain(-1.0)
    k_stop, eps = _stop_eps(free[2], free[3])
    obj = acc.DOptimalObj(V)
    kw = dict(logdet_refresh=0) if away else {}
    for e, length in ((eps, k_stop + 1), (1e30, 1)):
        ref = chain(e)
        assert len(ref[1]) == length
        want = (acc.D_opt_FW_away if away else acc.D_opt_FW)(obj, x0, e, 60, verbose=False, **kw)
        state = _obj_state(L, obj)
        got = (acc.D_opt_FW_away_device if away else acc.D_opt_FW_device)(obj, x0, e, 60, verbose=False, sync_every=7, **kw)
        _same(got[:4], want[:4], (away, e))
        _same(_obj_state(L, obj), state, (away, e, "state"))
        _same((got[0], got[2], got[3]), (ref[0], ref[2], ref[3]), (away, e, "NumPy"))
        _same(state, ref[5], (away, e, "NumPy state"))
    # through the C-ABI: the records behind the stop read "not run", and a later call goes on from the state
    with Dev(L, V) as dev:
        dev.init(x0)
        nsteps = k_stop + 4
        rc, nrun, recs = run_chunk(L, dev, away, eps, nsteps)
        assert rc == L.OK and nrun == k_stop + 1
        assert [r[-1] for r in recs] == [APPLIED] * k_stop + [STOPPED] + [NOT_RUN] * 3
        assert [(r[0], r[1]) for r in recs[:nrun]] == chain(eps)[4]
        _same(dev.state(), chain(eps)[5])
        rc, nrun, recs2 = run_chunk(L, dev, away, -1.0, 60 - k_stop)
        assert rc == L.OK and nrun == 60 - k_stop
        assert [(r[0], r[1]) for r in recs[:k_stop] + recs2] == free[4]
        _same(dev.state(), free[5])


# ------------------------------------------------------------------------------------- shapes where the paths fork
def test_housing_odd_m(acc):
    """(13, 506): the scalar paths of gemv_h and rank1"""
    V = golden("housing")["V"]
    n = V.shape[1]
    x0 = np.ones(n) / n
    obj = acc.DOptimalObj(V)
    _same(acc.D_opt_FW_device(obj, x0, 1e-9, 200, verbose=False)[:4], acc.D_opt_FW(obj, x0, 1e-9, 200, verbose=False)[:4])
    _same(acc.D_opt_FW_away_device(obj, x0, 1e-9, 200, verbose=False)[:4],
          acc.D_opt_FW_away(obj, x0, 1e-9, 200, verbose=False)[:4])


@pytest.mark.parametrize("n", [4095, 4097, 4608])
@pytest.mark.parametrize("away", [0, 1])
def test_either_side_of_the_sliced_away_search(L, n, away):
    """m = 16; the away variant's second stage is one workgroup below n = 4096 and sliced from there"""
    V = gaussian_design(16, n, 40 + n)
    _both_paths(L, V, np.ones(n) / n, away, 1e-9, [7, 1, 25], what=(n, away))


@pytest.mark.parametrize("away", [0, 1])
def test_padded_rows(L, away):
    """(37, 203) with ldv = 208 (padded rows, still 16-byte aligned: paired loads up to the odd last column) and
    ldv = 205 (vec_ok false: the scalar loads); the padding holds NaN"""
    V = gaussian_design(37, 203, 12)
    _both_paths(L, V, np.ones(203) / 203, away, 1e-9, [7, 23], ldv=208, what=("ldv", away))
    _both_paths(L, V, np.ones(203) / 203, away, 1e-9, [7, 23], ldv=205, what=("odd ldv", away))


@pytest.mark.parametrize("m,n", [(37, 203), (16, 4608)])
@pytest.mark.parametrize("away", [0, 1])
def test_mixed_with_the_step_calls(L, m, n, away):
    """accbpg_fw_run for 5 steps, 3 probe / update pairs, accbpg_fw_run for 5 more, against 13 steps one at a time: the
    stage-1 records that an update leaves for the next probe pass between the two interfaces both ways."""
    V = gaussian_design(m, n, 77)
    x0 = np.ones(n) / n
    a, b = _two(L, V, x0)
    with a, b:
        seq, mid = Sequential(L, b, away), Sequential(L, a, away)
        rc, want = seq.steps(1e-9, 13)
        rc1, n1, r1 = run_chunk(L, a, away, 1e-9, 5)
        mid.k = 5
        rc2, r2 = mid.steps(1e-9, 3)
        rc3, n3, r3 = run_chunk(L, a, away, 1e-9, 5)
        assert (rc, rc1, rc2, rc3, n1, n3) == (L.OK,) * 4 + (5, 5)
        _records_equal(r1 + r2 + r3, want, (m, n, away))
        _same(a.state(), b.state())
        # and a probe with the other support threshold right behind a run: stage 1 is taken afresh
        pa, pb = a.probe(1 - away), b.probe(1 - away)
        assert (pa.i, pa.j) == (pb.i, pb.j)
        np.testing.assert_array_equal([pa.w_i, pa.w_j, pa.x_j, pa.q_prev], [pb.w_i, pb.w_j, pb.x_j, pb.q_prev])


def test_arguments(L):
    V = gaussian_design(8, 40, 11)
    with Dev(L, V) as dev:
        assert run_chunk(L, dev, 0, 0.0, 4)[0] == L.ERR_ARG                     # no Frank-Wolfe state yet
        dev.init(np.ones(40) / 40)
        x, w, H = dev.state()
        for bad in (0, -1, 1025):
            steps = (L.FwStep * 1)()
            nrun = C.c_int(0)
            assert dev.lib.accbpg_fw_run(dev.h, 0, 0.0, bad, steps, C.byref(nrun)) == L.ERR_ARG
        _same(dev.state(), (x, w, H))
        rc, nrun, recs = run_chunk(L, dev, 0, -1.0, 1024)
        assert rc == L.OK and nrun == 1024 and recs[-1][-1] == APPLIED


# ------------------------------------------------------------------------------------- empty support, NaN
@pytest.mark.parametrize("n", [203, 4097])
def test_support_below_the_away_threshold(L, n):
    """The away variant from a support driven below 1e-8 by x-only updates.  Every d_k = (w_k - w_i) * 0 is a zero and
    the away index is 0, as NumPy gives: the step-by-step path takes that step without an error, and so must this
    one -- same records, same return code, same state.  (A pivot outside [0, n), status 2, cannot come out of the probe
    kernels as they stand; tests/test_fw_device_cpu.py covers the host's side of it.)"""
    m, start = _shape(n)
    s, x0 = N.axis_base(m, n, start)
    s[70], s[64] = 2.0, 0.25
    V, G = N.axis_design(m, n, s, x0)
    prepare = lambda dev: _shape_support(dev, [(64, 1.0e-8)])
    _both_paths(L, V, x0, 1, 1e-9, [1, 6], prepare=prepare, what=("empty support", n))
    a, b = _two(L, V, x0, prepare=prepare)
    with a, b:
        pr = b.probe(1)
        assert (pr.i, pr.j) == (70, 0) and pr.x_j == 0.0
        rc, nrun, first = run_chunk(L, a, 1, 1e-9, 1)
        assert rc == L.OK and first[0][:2] == (70, 0)


@pytest.mark.parametrize("n", [203, 4097])
@pytest.mark.parametrize("away", [0, 1])
def test_nan_falls_through_the_comparisons_as_in_python(L, n, away):
    """w all NaN (an update with hcoef = NaN), and one NaN behind a seam, planted as
    test_gpu_fw_steps.test_total_ties_and_non_finite_values plants them: neither the stop test nor eps_pos >= eps_neg
    holds for a NaN, on either side."""
    m, start = _shape(n)
    s, x0 = N.axis_base(m, n, start)
    V, G = N.axis_design(m, n, s, x0)
    all_nan = lambda dev: dev.update(start + 3, 1.0, 0.0, NAN, 1.0)
    recs = _both_paths(L, V, x0, away, 1e30, [3, 2], prepare=all_nan, what=("all nan", n, away))
    assert np.isnan(recs[0][2]) and recs[0][-1] == APPLIED and recs[0][-2] == (1 if away else 0)
    k = 256 if n > 256 else 64
    r, p = k % m, k + 3 * m
    s, x0 = N.axis_base(m, n, start)
    x0[(np.arange(n) % m == r)] = 0.0
    s[k], x0[k] = 2.0 ** 500, 2.0 ** -1004
    s[p] = 2.0 ** 8
    V, G = N.axis_design(m, n, s, x0)

    def one_nan(dev):
        dev.update(p, 1.0, 0.25, 1.0, 1.0)
        dev.update(p, 1.0, 0.0, -2.0 ** -40, 1.0)
        x, w, H = dev.state()
        assert np.isnan(w[k]) and np.all(np.isfinite(np.delete(w, k)))

    _both_paths(L, V, x0, away, 1e30, [3, 2], prepare=one_nan, what=("one nan", n, away))
