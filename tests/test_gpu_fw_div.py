"""The Bregman-step Frank-Wolfe solvers on the maintained state (D_opt_FW_div_step, D_opt_FW_descent_step) and their two
C-ABI calls (accbpg_fw_div_probe_step, accbpg_fw_div_apply) on the device.  References: the state read back through
accbpg_fw_get_state, tests/reduce_numpy.py for the fixed summation tree (block cap 512), np.longdouble sums with the
forward bound (tree_depth + c) EPS sum|terms| (c roundings per term), tests/fw_numpy.py for one update (the bounds of
tests/test_gpu_fw_steps.py), tests/fwdiv_numpy.py for whole runs, the generic solvers of the package, and the real
reference's traces under tests/golden.

Shapes: housing (13,506), (16,257), (80,200), (64,512), (32,4097), (128,2049): either side of the 256-thread block,
of the 512-column group of the pass over V and of the first multi-block reduction (1024 entries per block).

The bound on sum_u2 has one more part: the device's u = V^T (H v_i) is itself a rounded quantity,
|u_k - u_k(exact)| <= gamma(2m) B_k (tests/test_gpu_fw_steps.py), so each term u_k^2 moves by at most
gamma(2m + 1) (2 |u_k| B_k + gamma(2m + 1) B_k^2) before the tree adds it."""
import ctypes as C
import os

import numpy as np
import pytest

import fw_numpy as N
import fwdiv_numpy as R
import reduce_numpy as T
from conftest import gaussian_design
from test_gpu_fw_steps import NOOP, Dev, _axis_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOUSING = os.path.join(ROOT, "tests", "golden", "data", "housing.txt")
CAP = 512                               # FW_DIV_CAP
FILL = 1e-15
SHAPES = ["housing", (16, 257), (80, 200), (64, 512), (32, 4097), (128, 2049)]
SEEDS = {(16, 257): 2, (80, 200): 10, (64, 512): 3, (32, 4097): 7, (128, 2049): 5}


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


def _design(acc, shape):
    if shape == "housing":
        return np.ascontiguousarray(acc.D_opt_libsvm(HOUSING)[0].H)
    m, n = shape
    return gaussian_design(m, n, 500 + m + n)


def _probe(dev, value=1.0, fill=FILL, ok=True):
    rec = dev.L.FwDivProbe()
    rc = dev.lib.accbpg_fw_div_probe_step(dev.h, float(fill), float(value), C.byref(rec))
    if ok:
        assert rc == dev.L.OK, dev.L.last_error()
    return rec


def _apply(dev, p, a, value, hcoef, hdiv, fill=FILL):
    return dev.lib.accbpg_fw_div_apply(dev.h, int(p), float(a), float(fill), float(value), float(hcoef), float(hdiv))


def _random_x(n, seed):
    x = np.random.RandomState(seed).rand(n) + 0.05
    return x / x.sum()


def _within(got, terms, c, n, what, extra=0.0):
    terms = np.asarray(terms, dtype=np.longdouble)
    exact = np.sum(terms)
    bound = (T.tree_depth(n, CAP) + c) * T.EPS * float(np.sum(np.abs(terms))) + extra
    err = abs(float(np.longdouble(got) - exact))
    print("%-8s err %.3e bound %.3e ratio %.4f" % (what, err, bound, err / bound))
    assert err <= bound, (what, got, float(exact), err, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_probe_record(acc, L, shape):
    V = _design(acc, shape)
    m, n = V.shape
    value = 1.0 if shape != (80, 200) else 2.5
    with Dev(L, V) as dev:
        dev.init(_random_x(n, n))
        for fused in (False, True):
            if fused:                                           # stage 1 comes with the w pass of an update
                dev.update(*NOOP)
            x, w, H = dev.state()
            rec = _probe(dev, value)
            i = int(np.argmin(-w))
            assert rec.i == i and rec.w_i == w[i] and rec.x_i == x[i] and rec.min_x == x.min()
            assert rec.sum_w == T.tree_sum(w, CAP)
            wl, xl = w.astype(np.longdouble), x.astype(np.longdouble)
            s = np.full(n, FILL, dtype=np.longdouble)
            s[i] = value
            _within(rec.sum_w2, wl * wl, 2, n, "sum_w2")
            _within(rec.slope, (-wl) * (s - xl), 2, n, "slope")
            r = s / xl
            _within(rec.div, r - np.log(r) - 1, 4, n, "div")
            ref = N.update_ref(V, H, w, i, 0.0, 1.0)
            g = N.gamma(2 * m + 1)
            moved = float(np.sum(g * (2 * np.abs(ref.u) * ref.B + g * ref.B ** 2)))
            _within(rec.sum_u2, ref.u * ref.u, 2, n, "sum_u2", extra=moved)
            again = _probe(dev, value)
            for name, _ in L.FwDivProbe._fields_:
                assert getattr(again, name) == getattr(rec, name), name


@pytest.mark.parametrize("a,b", [(255, 256), (2047, 2048), (63, 64)])
def test_first_index_on_ties_across_seams(L, a, b):
    m, n, start = 16, 4097, 1024
    for kind in ("tie", "twin"):
        s, x0 = N.axis_base(m, n, start)
        s[a], s[b] = 2.0, (2.0 if kind == "tie" else 4.0)
        dev, V, G = _axis_dev(L, m, n, s, x0)
        with dev:
            want = a if kind == "tie" else b
            for fused in (False, True):
                if fused:
                    dev.update(*NOOP)
                rec = _probe(dev)
                assert rec.i == want and rec.w_i == (64.0 if kind == "tie" else 256.0), (kind, fused, rec.i)
                assert rec.min_x == 0.0 and rec.x_i == 0.0


def test_nan_in_w_is_picked_as_argmin_picks_it(L):
    """the one-NaN construction of test_gpu_fw_steps.test_total_ties_and_non_finite_values, behind the seam 255|256"""
    m, n, start = 16, 4097, 1024
    k = 256
    p = k + 3 * m
    s, x0 = N.axis_base(m, n, start)
    x0[(np.arange(n) % m == k % m)] = 0.0
    s[k], x0[k] = 2.0 ** 500, 2.0 ** -1004
    s[p] = 2.0 ** 8
    dev, V, G = _axis_dev(L, m, n, s, x0)
    with dev:
        dev.update(p, 1.0, 0.25, 1.0, 1.0)
        dev.update(p, 1.0, 0.0, -2.0 ** -40, 1.0)
        x, w, _ = dev.state(with_H=False)
        assert np.isnan(w[k]) and np.all(np.isfinite(np.delete(w, k)))
        for _ in range(2):                                      # fused stage 1, then fresh
            rec = _probe(dev)
            assert rec.i == int(np.argmin(-w)) == k and np.isnan(rec.w_i) and np.isnan(rec.sum_w)


def test_nonpositive_x_raises(acc):
    f, h, L0, x0 = acc.D_opt_design(16, 257, randseed=2)
    x0 = x0.copy()
    x0[200] = 0.0
    with pytest.raises(AssertionError):
        acc.D_opt_FW_div_step(f, L0, x0, 3, 2.0, verbose=False)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_one_apply(acc, L, shape):
    from accbpg_and_fw_amd.functions import vec_axpby, vec_vertex
    V = _design(acc, shape)
    m, n = V.shape
    g = N.gamma
    with Dev(L, V) as dev:
        ld = dev.init(_random_x(n, n + 1))
        rec = _probe(dev)
        x, w, H = dev.state()
        a = 0.3
        hcoef, hdiv, ld1, q1, f1 = R.step_scalars(a, 1.0, dict(w_i=rec.w_i, sum_w=rec.sum_w, sum_u2=rec.sum_u2), ld, 0.0, m)
        # a pivot that is not the probe's: refused, nothing moves
        assert _apply(dev, (rec.i + 1) % n, a, 1.0, hcoef, hdiv) == L.ERR_ARG
        for got, exp in zip(dev.state(), (x, w, H)):
            np.testing.assert_array_equal(got, exp)
        assert _apply(dev, rec.i, a, 1.0, hcoef, hdiv) == L.OK, L.last_error()
        x1, w1, H1 = dev.state()
        xd = torch.from_numpy(x).cuda()
        d = vec_axpby(1.0, vec_vertex(rec.i, 1.0, FILL, n, xd.device), -1.0, xd)
        np.testing.assert_array_equal(x1, vec_axpby(1.0, xd, a, d).cpu().numpy())
        ref = N.update_ref(V, H, w, rec.i, hcoef, hdiv)
        bH = g(2 * m + 5) * (np.abs(H) + abs(hcoef) * np.outer(ref.A, ref.A)) / abs(hdiv)
        bw = g(4 * m + 5) * (np.abs(w) + abs(hcoef) * ref.B ** 2) / abs(hdiv)
        rH = float(np.max(np.abs(H1 - ref.H) / bH))
        rw = float(np.max(np.abs(w1 - ref.w) / bw))
        print("ratio to bound H' %.4f w' %.4f" % (rH, rw))
        assert rH <= 1.0 and rw <= 1.0
        assert np.max(np.abs(w1 - w) / bw) > 1e3 and np.max(np.abs(H1 - H) / bH) > 1e3
        # the trial value of the line search is the value at the point the apply reached
        fx = acc.DOptimalObj(V)(x1)
        assert abs(f1 - fx) <= 1e-10 * max(1.0, abs(fx)), (f1, fx)
        # a second apply without a probe in between: refused
        assert _apply(dev, rec.i, a, 1.0, hcoef, hdiv) == L.ERR_ARG
        # the stage-1 records the apply left serve the existing probe as well
        x2, w2, _ = dev.state(with_H=False)
        pr = dev.probe(0)
        assert pr.i == int(np.argmax(w2)) and pr.w_i == w2.max()


def _prefix(a, b, tol=1e-12):
    n = min(len(a), len(b))
    bad = np.nonzero(np.abs(a[:n] - b[:n]) > tol * (1 + np.abs(b[:n])))[0]
    return n if bad.size == 0 else int(bad[0])


def _instance(acc, shape):
    if shape == "housing":
        return acc.D_opt_libsvm(HOUSING)
    return acc.D_opt_design(shape[0], shape[1], randseed=SEEDS[shape])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_trajectories(acc, shape):
    f, h, L0, x0 = _instance(acc, shape)
    V = np.ascontiguousarray(f.H)
    x, F, Ls, Tm = acc.D_opt_FW_div_step(f, L0, x0, 300, 2.0, verbose=False)
    assert isinstance(x, np.ndarray) and len(F) == len(Ls) == len(Tm)
    xr, Fr, Lsr = R.fw_div_step(V, L0, x0, 300, 2.0)
    xg, Fg, Lsg, _ = acc.FW_alg_div_step(f, h, L0, x0, 300, 2.0, acc.lmo_simplex(), verbose=False)
    for name, Fo, Lso in (("restatement", Fr, Lsr), ("generic", Fg, Lsg)):
        k = _prefix(Ls, Lso)
        dev = float(np.max(np.abs(F[:k] - Fo[:k]) / np.maximum(1, np.abs(Fo[:k]))))
        print("div step  %-11s %s prefix %d F dev %.3e" % (name, shape, k, dev))
        assert k >= 150, (name, k)
        np.testing.assert_allclose(F[:k], Fo[:k], rtol=1e-9, atol=1e-9)
    x, F, Tm, G = acc.D_opt_FW_descent_step(f, x0, 300, verbose=False)
    assert len(F) == len(Tm) == len(G) and not G.any()
    xr, Fr = R.fw_descent_step(V, x0, 300)
    xg, Fg, _, _ = acc.FW_alg_descent_step(f, h, x0, 300, acc.lmo_simplex(), verbose=False)
    for name, Fo, xo in (("restatement", Fr, xr), ("generic", Fg, xg)):
        assert len(F) == len(Fo), name
        dev = float(np.max(np.abs(F - Fo) / np.maximum(1, np.abs(Fo))))
        print("descent   %-11s %s F dev %.3e x dev %.3e" % (name, shape, dev, np.max(np.abs(x - xo))))
        np.testing.assert_allclose(F, Fo, rtol=1e-9, atol=1e-9)


def test_goldens(acc):
    nr = np.load(os.path.join(ROOT, "tests", "golden", "next_rows.npz"))
    gd = np.load(os.path.join(ROOT, "tests", "golden", "fwdiv.npz"))
    for tag, inst in (("h", acc.D_opt_libsvm(HOUSING)), ("r", acc.D_opt_design(80, 200, randseed=10))):
        f, h, L0, x0 = inst
        x, F, Ls, _ = acc.D_opt_FW_div_step(f, L0, x0, 300, 2.0, ls_ratio=2, verbose=False)
        k = _prefix(Ls, nr[tag + "_fwdiv_Ls"])
        print("golden div step %s prefix %d" % (tag, k))
        assert k >= 150, k
        np.testing.assert_allclose(F[:k], nr[tag + "_fwdiv_F"][:k], rtol=1e-9, atol=1e-9)
        x, F, _, _ = acc.D_opt_FW_descent_step(f, x0, 300, verbose=False)
        print("golden descent %s F dev %.3e" % (tag, np.max(np.abs(F - gd[tag + "_desc_F"][:300]))))
        np.testing.assert_allclose(F, gd[tag + "_desc_F"][:300], rtol=1e-9, atol=1e-9)


def test_refresh(acc):
    f, h, L0, x0 = acc.D_opt_design(32, 300, randseed=6)
    x0_, F0, Ls0, _ = acc.D_opt_FW_div_step(f, L0, x0, 40, 2.0, verbose=False, refresh=0)
    x5, F5, Ls5, _ = acc.D_opt_FW_div_step(f, L0, x0, 40, 2.0, verbose=False, refresh=5)
    np.testing.assert_array_equal(Ls5, Ls0)
    np.testing.assert_allclose(F5, F0, rtol=1e-10, atol=1e-10)
    # right after a refresh w is minus the gradient of a fresh objective at x
    from accbpg_and_fw_amd.D_opt_alg import _FWDivState
    st = _FWDivState(f, x0, 1, 5)
    for _ in range(5):
        rec = st.probe_div()
        hcoef, hdiv, ld1, q1, _f1 = st.scalars(0.3, rec)
        st.apply(rec, 0.3, hcoef, hdiv, ld1, q1)
    assert st.since == 5 and st.q > 0
    st.refresh_if_due()
    assert st.since == 0 and st.q == 0.0
    xd, wd, _ = st.state()
    fresh = acc.DOptimalObj(np.ascontiguousarray(f.H))
    np.testing.assert_allclose(wd.cpu().numpy(), -fresh.gradient(xd.cpu().numpy()), rtol=1e-9)
    assert abs(st.ld + fresh(xd.cpu().numpy())) <= 1e-10 * max(1.0, abs(st.ld))


def test_capped_step_reinitialises(acc):
    """linesearch=False and a tiny L: a = 1.0, the iterate jumps to the vertex and the state is recomputed from it."""
    f, h, L0, x0 = acc.D_opt_design(16, 257, randseed=2)
    args = dict(linesearch=False, verbose=False)
    try:
        xg, Fg, Lsg, _ = acc.FW_alg_div_step(f, h, 1e-12, x0, 3, 2.0, acc.lmo_simplex(), **args)
    except ValueError:
        print("capped step: the vertex is singular in both")
        with pytest.raises(ValueError):
            acc.D_opt_FW_div_step(f, 1e-12, x0, 3, 2.0, **args)
        return
    x, F, Ls, _ = acc.D_opt_FW_div_step(f, 1e-12, x0, 3, 2.0, **args)
    print("capped step: F", F, "generic", Fg)
    assert len(F) == len(Fg)
    np.testing.assert_allclose(F, Fg, rtol=1e-9)


def test_rejected_capped_trials_then_a_rank_one_step(acc):
    """A tiny L with the line search on: the first trials sit at the cap a = 1 and are evaluated in full (and rejected),
    L doubles until a < 1, and the accepted step is applied with the direction of the one probe."""
    f, h, L0, x0 = acc.D_opt_design(16, 257, randseed=2)
    xg, Fg, Lsg, _ = acc.FW_alg_div_step(f, h, 1e-9, x0, 12, 2.0, acc.lmo_simplex(), verbose=False)
    x, F, Ls, _ = acc.D_opt_FW_div_step(f, 1e-9, x0, 12, 2.0, verbose=False)
    assert Ls[0] > 1e-6                                         # many doublings in the first iteration
    np.testing.assert_array_equal(Ls, Lsg)
    np.testing.assert_allclose(F, Fg, rtol=1e-9)
    np.testing.assert_allclose(x, xg, rtol=0, atol=1e-11)


def test_two_runs_are_bit_identical_and_tensors_stay_tensors(acc):
    f, h, L0, x0 = acc.D_opt_design(64, 512, randseed=3)
    a = acc.D_opt_FW_div_step(f, L0, x0, 60, 2.0, verbose=False)
    b = acc.D_opt_FW_div_step(np.ascontiguousarray(f.H), L0, x0, 60, 2.0, verbose=False)
    for u, v in zip(a[:3], b[:3]):
        np.testing.assert_array_equal(u, v)
    a = acc.D_opt_FW_descent_step(f, x0, 60, verbose=False)
    b = acc.D_opt_FW_descent_step(f, x0, 60, verbose=False)
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])
    xt = torch.from_numpy(x0).cuda()
    x, F, Ls, _ = acc.D_opt_FW_div_step(f, L0, xt, 60, 2.0, verbose=False)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    np.testing.assert_array_equal(x.cpu().numpy(), acc.D_opt_FW_div_step(f, L0, x0, 60, 2.0, verbose=False)[0])
    x, F, _, _ = acc.D_opt_FW_descent_step(f, xt, 60, verbose=False)
    assert isinstance(x, torch.Tensor) and x.is_cuda
    np.testing.assert_array_equal(x.cpu().numpy(), a[0])
