"""The Frank-Wolfe step kernels one step at a time, on a single handle through the C-ABI (``accbpg_fw_init``,
``accbpg_fw_probe_step``, ``accbpg_fw_update``, ``accbpg_fw_get_state``, ``accbpg_dopt_vt_times``,
``accbpg_dopt_get_column``) and, at the end, through the lock-step wrappers.  The reference is tests/fw_numpy.py (the
step restated from the reference algorithm, pinned to the oracle by tests/test_fw_step_cpu.py), never another kernel.

Two kinds of input:

* AXIS DESIGNS (column k = s_k e_{k mod m}, s_k and x0 dyadic, every G_rr an even power of two): the Gram matrix, its
  factor, W, H and every later H' are diagonal and every sum in every kernel has at most one nonzero term (the Gram
  entries: only exact partial sums), so the result cannot depend on summation order, partition, or fma against
  mul + add -- the float64 restatement must match the device to the LAST BIT, for any scalars, over any number of
  steps.  Each test first asserts that precondition on the device: H == diag(1/G_rr) and w == s^2 / G_rr exactly after
  ``accbpg_fw_init``.  On these the probe decisions are planted: ties on either side of every seam of the two-stage
  searches, the two support thresholds, the away index taken on rounded differences, total ties, NaN.

* GAUSSIAN DESIGNS: one update against ``fw_numpy.update_ref`` (np.longdouble) within forward bounds derived below.

Seams (from the launch constants: 256 threads per workgroup, 8 * 256 columns per fresh stage-1 workgroup, at most 512
stage-1 workgroups, at most 128 away slices, two-stage away search from n = 4096): a lane boundary 63|64, a workgroup
boundary 255|256, a fresh stage-1 boundary 2047|2048, the away slice boundary of each n, and where the fused stage 1
wraps round its 512 workgroups (131071|131072).

The forward bounds.  u = 2^-53, gamma(c) = c u / (1 - c u).  A length-m dot product evaluated in ANY order, with or
without fma, passes each term through at most m roundings (its product and at most m - 1 additions; adding to an exact
zero is free), so |fl(a.b) - a.b| <= gamma(m) sum |a_r||b_r|.  With A = |H||v_p| (so |Hv_r| <= A_r):
    Hv_r                 gamma(m) A_r
    q = v_p.Hv           gamma(2m) Q,  Q = |v_p|.A           (m roundings of its own on top of those of Hv)
    H'_rc                gamma(2m+4) (|H_rc| + |hcoef| A_r A_c) / |hdiv|
                         (each factor of the outer product carries gamma(m); then product, times hcoef, sum, quotient)
    u_k = Hv.V[:,k]      gamma(2m) B_k,  B_k = sum_r A_r |V_rk|
    w'_k                 gamma(4m+4) (|w_k| + |hcoef| B_k^2) / |hdiv|     (u_k^2 doubles the 2m; then the same four)
    V^T q (given q)      gamma(m) sum_r |q_r||V_rk|
One more rounding is granted throughout for the np.longdouble reference's own error (2^-64 per operation, far below
one float64 rounding in total).  Nothing here is fitted to what the kernels return; DESIGN.md section 7 records the
largest observed ratio to each bound."""
import ctypes as C

import numpy as np
import pytest

import fw_numpy as N
from conftest import gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FB, FRESH_COLS, STAGE1_CAP, AWAY_NB, AWAY_TWO_STAGE = 256, 8 * 256, 512, 128, 4096
INF, NAN = float("inf"), float("nan")


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


class Dev:
    """One D-optimal handle made through the C-ABI on a matrix with row stride ``ldv`` (the padding holds NaN: a
    kernel that reads it shows)."""

    def __init__(self, L, V, ldv=None):
        self.L, self.lib = L, L.load()
        self.m, self.n = V.shape
        ldv = self.n if ldv is None else ldv
        self.buf = torch.full((self.m, ldv), NAN, dtype=torch.float64, device="cuda")
        self.buf[:, :self.n] = torch.from_numpy(np.ascontiguousarray(V))
        self.h = C.c_void_p()
        rc = self.lib.accbpg_dopt_create(C.c_void_p(self.buf.data_ptr()), self.m, self.n, ldv, self._stream(),
                                         C.byref(self.h), 0 if self.m < self.n else 1)
        assert rc == L.OK, L.last_error()

    @staticmethod
    def _stream():
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def close(self):
        if self.h:
            torch.cuda.synchronize()
            self.lib.accbpg_dopt_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def init(self, x0):
        x0d = torch.from_numpy(np.ascontiguousarray(x0, dtype=np.float64)).cuda()
        ld = C.c_double(0.0)
        rc = self.lib.accbpg_fw_init(self.h, C.c_void_p(x0d.data_ptr()), C.byref(ld))
        assert rc == self.L.OK, self.L.last_error()
        return ld.value

    def probe(self, away, refresh=0):
        pr = self.L.FwProbe()
        assert self.lib.accbpg_fw_probe_step(self.h, int(away), int(refresh), C.byref(pr)) == self.L.OK
        return pr

    def update(self, p, xscale, xadd, hcoef, hdiv):
        rc = self.lib.accbpg_fw_update(self.h, int(p), float(xscale), float(xadd), float(hcoef), float(hdiv))
        assert rc == self.L.OK, self.L.last_error()

    def state(self, with_H=True):
        x = torch.empty(self.n, dtype=torch.float64, device="cuda")
        w = torch.empty(self.n, dtype=torch.float64, device="cuda")
        H = torch.empty(self.m, self.m, dtype=torch.float64, device="cuda") if with_H else None
        rc = self.lib.accbpg_fw_get_state(self.h, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                          C.c_void_p(H.data_ptr()) if with_H else None)
        assert rc == self.L.OK
        return x.cpu().numpy(), w.cpu().numpy(), (H.cpu().numpy() if with_H else None)

    def vt_times(self, q):
        qd = torch.from_numpy(np.ascontiguousarray(q)).cuda()
        u = torch.full((self.n,), NAN, dtype=torch.float64, device="cuda")
        assert self.lib.accbpg_dopt_vt_times(self.h, C.c_void_p(qd.data_ptr()), C.c_void_p(u.data_ptr())) == self.L.OK
        torch.cuda.synchronize()
        return u.cpu().numpy()

    def column(self, j):
        out = torch.full((self.m,), NAN, dtype=torch.float64, device="cuda")
        assert self.lib.accbpg_dopt_get_column(self.h, int(j), C.c_void_p(out.data_ptr())) == self.L.OK
        torch.cuda.synchronize()
        return out.cpu().numpy()


def _axis_dev(L, m, n, s, x0):
    """A handle on the axis design (s, x0), initialised, with the exactness precondition asserted ON THE DEVICE:
    H == diag(1/G_rr) and w == s^2 / G_rr to the bit (a failure here is a finding about the init path: Gram,
    Cholesky, triangular inverse, column norms)."""
    G = np.array(N.axis_exact(m, s, x0))
    V, Gd = N.axis_design(m, n, s, x0)
    np.testing.assert_array_equal(Gd, G)
    dev = Dev(L, V)
    _axis_init(dev, m, n, s, x0, G)
    return dev, V, G


def _axis_init(dev, m, n, s, x0, G):
    logdet = dev.init(x0)
    x, w, H = dev.state()
    np.testing.assert_array_equal(x, x0)
    np.testing.assert_array_equal(H, np.diag(1.0 / G))
    np.testing.assert_array_equal(w, s * s / G[np.arange(n) % m])
    assert abs(logdet - np.sum(np.log(G))) <= 1e-12 * (1 + abs(np.sum(np.log(G))))


def _rec_equal(got, exp, what):
    """every field of a probe record, exactly (NaN equals NaN)"""
    assert (got.i, got.j) == (exp.i, exp.j), (what, (got.i, got.j, got.w_i, got.w_j, got.x_j), exp)
    np.testing.assert_array_equal([got.w_i, got.w_j, got.x_j], [exp.w_i, exp.w_j, exp.x_j], err_msg=str(what))


NOOP = (0, 1.0, 0.0, 0.0, 1.0)          # x * 1, x[0] += 0, H and w: (. + 0 * .) / 1


def _check_probes(dev, what, expect=None):
    """Both probe variants against fw_numpy.probe on the downloaded (w, x): the probe as it comes, a FRESH probe (no
    stage-1 records are left after a probe), and a probe that PICKS UP the stage-1 records that an update -- here one
    that changes nothing -- fused with its w pass.  ``expect``: {away: (i, j)} the planted outcome."""
    for away in (0, 1):
        x, w, _ = dev.state(with_H=False)
        exp = N.probe(w, x, away)
        if expect is not None:
            assert (exp.i, exp.j) == tuple(expect[away]), (what, away, exp, expect[away])
        _rec_equal(dev.probe(away), exp, (what, away, "as it comes"))
        _rec_equal(dev.probe(away), exp, (what, away, "fresh"))
        dev.update(*NOOP)
        x2, w2, _ = dev.state(with_H=False)
        np.testing.assert_array_equal(x2, x)
        np.testing.assert_array_equal(w2, w)
        _rec_equal(dev.probe(away), exp, (what, away, "fused stage 1"))


# ---------------------------------------------------------------------------------------------- a. probe decisions
PROBE_N = [40, 203, 4095, 4096, 4097, 4608, 131072 + 257, 262144 + 2049]


def _shape(n):
    """(m, first base column) of the planted designs at this n"""
    return {40: (8, 8), 203: (8, 100)}.get(n, (16, 1024))


def _away_per(n):
    nb2 = min((n + FRESH_COLS - 1) // FRESH_COLS, AWAY_NB)
    return (n + nb2 - 1) // nb2


def _seams(n):
    """index pairs (a, b), a < b, on either side of each seam that exists at this n, clear of the base columns"""
    m, start = _shape(n)
    pairs = [(2, 5)] if n == 40 else [(63, 64)]
    pairs += [(255, 256), (FRESH_COLS - 1, FRESH_COLS)]
    if n >= AWAY_TWO_STAGE:
        per = _away_per(n)
        pairs += [(per - 1, per), (3 * per - 1, 3 * per)]
    wrap = STAGE1_CAP * FB
    if n > wrap:
        pairs += [(wrap - 1, wrap), (300, wrap + 5), (wrap + 255, wrap + 256)]
    if n > 2 * wrap:
        pairs += [(2 * wrap - 1, 2 * wrap), (wrap + 7, 2 * wrap + 3)]
    ok = []
    for a, b in pairs:                                  # (at n = 4096 the away slice boundary IS 2047|2048)
        if b < n and (a, b) not in ok and not (start <= a < start + 4 * m) and not (start <= b < start + 4 * m):
            ok.append((a, b))
    assert len(ok) >= 3 or n < 4095
    return ok


def _shape_support(dev, points):
    """x = sum of c e_p over ``points`` exactly, through updates that touch only x"""
    first = True
    for p, c in points:
        dev.update(p, 0.0 if first else 1.0, c, 0.0, 1.0)
        first = False


def test_x_only_update_leaves_w_and_H_bit_unchanged(L):
    m, n = 16, 4097
    s, x0 = N.axis_run_design(m, n, 1024)
    dev, V, G = _axis_dev(L, m, n, s, x0)
    with dev:
        x, w, H = dev.state()
        dev.update(77, 1.0, 0.125, 0.0, 1.0)
        x1, w1, H1 = dev.state()
        np.testing.assert_array_equal(w1, w)
        np.testing.assert_array_equal(H1, H)
        np.testing.assert_array_equal(x1, N.update_x(x, 77, 1.0, 0.125))
        dev.update(5, 0.0, 0.25, 0.0, 1.0)
        x2, w2, H2 = dev.state()
        np.testing.assert_array_equal(w2, w)
        np.testing.assert_array_equal(H2, H)
        e = np.zeros(n); e[5] = 0.25
        np.testing.assert_array_equal(x2, e)


@pytest.mark.parametrize("n", PROBE_N)
def test_planted_ties_across_seams(L, n):
    """Per seam (a | b): equal maximal w at a and b, and equal minimal supported w on either side of the NEXT seam (c | d)
    -- the lower index wins; and the twin in which the higher-index side is strictly better -- it wins.  All other
    w are 16, the support is {c, d, two ordinary columns}."""
    m, start = _shape(n)
    seams = _seams(n)
    for q, (a, b) in enumerate(seams):
        c, d = seams[(q + 1) % len(seams)]
        if len({a, b, c, d}) < 4:
            c, d = (0, 1)
        for kind in ("tie", "twin"):
            s, x0 = N.axis_base(m, n, start)
            s[a], s[b] = 2.0, (2.0 if kind == "tie" else 4.0)          # w = 64, 64 | 256
            s[c], s[d] = 0.5, (0.5 if kind == "tie" else 0.25)         # w = 4, 4 | 1
            dev, V, G = _axis_dev(L, m, n, s, x0)
            with dev:
                _shape_support(dev, [(c, 0.125), (d, 0.125), (start + 1, 0.25), (start + 4 * m - 1, 0.0625)])
                i = a if kind == "tie" else b
                j = c if kind == "tie" else d
                _check_probes(dev, (n, a, b, c, d, kind), {0: (i, j), 1: (i, j)})


@pytest.mark.parametrize("n", [203, 4097])
def test_support_threshold_edges(L, n):
    """x_k = 1e-8 exactly is inside the Frank-Wolfe support (x > 0) and outside the away support (x > 1e-8);
    nextafter(1e-8, 1) is inside both; x_k = 0 outside both.  Then the support reduced to the pivot alone: every
    d_k is +-0 and the away index is 0, as NumPy gives."""
    m, start = _shape(n)
    s, x0 = N.axis_base(m, n, start)
    a, c, d, z, e = 70, 64, 63, 3, start + 2
    s[a], s[c], s[d], s[z] = 2.0, 0.25, 0.5, 0.125                      # w = 64, 1, 4, 1/4 (others 16)
    dev, V, G = _axis_dev(L, m, n, s, x0)
    with dev:
        _shape_support(dev, [(c, 1.0e-8), (d, float(np.nextafter(1.0e-8, 1.0))), (e, 0.5)])
        x, w, _ = dev.state(with_H=False)
        assert x[c] == 1.0e-8 and x[d] == np.nextafter(1.0e-8, 1.0) and x[z] == 0.0 and w[z] == 0.25
        _check_probes(dev, (n, "edges"), {0: (a, c), 1: (a, d)})
        _shape_support(dev, [(a, 0.5)])
        _check_probes(dev, (n, "pivot alone"), {0: (a, a), 1: (a, 0)})
        _shape_support(dev, [(c, 1.0e-8)])                              # no away support at all: j = 0 again
        _check_probes(dev, (n, "below the away threshold"), {0: (a, c), 1: (a, 0)})


@pytest.mark.parametrize("n,lo,hi", [(203, 63, 64), (4097, 2047, 2048), (4608, 1535, 1536)])
def test_away_index_is_taken_on_rounded_differences(L, n, lo, hi):
    """w_i = 2^64; the supported columns have w = 16 (1 + 2^-19 + 2^-40) at the LOWER index and w = 16 at the higher:
    both differences round to -w_i, so the reference returns the lower index although its w is the larger one (the
    Frank-Wolfe variant, which compares w itself, returns the higher)."""
    m, start = _shape(n)
    s, x0 = N.axis_base(m, n, start)
    big = 200 if n > 203 else 20
    s[big] = 2.0 ** 30
    s[lo] = 1.0 + 2.0 ** -20
    dev, V, G = _axis_dev(L, m, n, s, x0)
    with dev:
        _shape_support(dev, [(lo, 0.25), (hi, 0.25)])
        x, w, _ = dev.state(with_H=False)
        assert w[big] == 2.0 ** 64 and w[lo] == 16 * (1 + 2.0 ** -19 + 2.0 ** -40) and w[hi] == 16.0
        assert w[lo] - w[big] == w[hi] - w[big] == -w[big]
        _check_probes(dev, (n, "collision"), {0: (big, hi), 1: (big, lo)})


@pytest.mark.parametrize("n", [203, 4097])
def test_total_ties_and_non_finite_values(L, n):
    """All w equal to 0, to inf, to NaN (made with the scalars of an update: hdiv = inf, hdiv = 0, hcoef = nan), and
    one NaN behind a seam: the expected record is what np.argmax / np.argmin return on the downloaded arrays (the
    first index on a total tie, the first NaN).  The handle is initialised again after each."""
    m, start = _shape(n)
    s, x0 = N.axis_base(m, n, start)
    G = np.array(N.axis_exact(m, s, x0))
    V, _ = N.axis_design(m, n, s, x0)
    with Dev(L, V) as dev:
        for name, hcoef, hdiv, value in (("zero", 0.0, INF, 0.0), ("inf", 0.0, 0.0, INF), ("nan", NAN, 1.0, NAN)):
            _axis_init(dev, m, n, s, x0, G)
            dev.update(start + 3, 1.0, 0.0, hcoef, hdiv)
            x, w, _ = dev.state(with_H=False)
            np.testing.assert_array_equal(w, np.full(n, value))
            np.testing.assert_array_equal(x, x0)
            for away in (0, 1):
                exp = N.probe(w, x, away)
                assert (exp.i, exp.j) == (0, 0 if away else start)
                _rec_equal(dev.probe(away), exp, (n, name, away, "first"))
                _rec_equal(dev.probe(away), exp, (n, name, away, "fresh"))
    # one NaN at k, behind a seam: w_k = 2^1004 becomes inf when u_k^2 overflows against hcoef = 1, then inf - inf
    # when it overflows against a negative hcoef.  Row r of k and of the pivot p holds no base column: k itself
    # carries it (x0_k = 2^-1004, inside the Frank-Wolfe support only).
    k = 256 if n > 256 else 64
    r = k % m
    p = k + 3 * m
    s, x0 = N.axis_base(m, n, start)
    x0[(np.arange(n) % m == r)] = 0.0
    s[k], x0[k] = 2.0 ** 500, 2.0 ** -1004
    s[p] = 2.0 ** 8
    dev, V, G = _axis_dev(L, m, n, s, x0)
    with dev:
        dev.update(p, 1.0, 0.25, 1.0, 1.0)
        x, w, _ = dev.state(with_H=False)
        assert w[k] == INF and np.all(np.isfinite(np.delete(w, k)))
        dev.update(p, 1.0, 0.0, -2.0 ** -40, 1.0)
        x, w, H = dev.state()
        assert np.isnan(w[k]) and np.all(np.isfinite(np.delete(w, k))) and np.all(np.isfinite(H)) and x[k] > 0
        for away in (0, 1):
            exp = N.probe(w, x, away)
            assert (exp.i, exp.j) == (k, 0 if away else k)
            _rec_equal(dev.probe(away), exp, (n, "one nan", away, "first"))
            _rec_equal(dev.probe(away), exp, (n, "one nan", away, "fresh"))


# ------------------------------------------------------------------------------------- b. whole runs, bit for bit
def _drive(dev, m, away, eps, maxitrs):
    """the solver's loop through the C-ABI (decisions by the package's own code), recording every (i, j)"""
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    picks = []
    run = _AwayRun(m, maxitrs, 0, 1)
    for k in range(maxitrs):
        pr = dev.probe(away)
        picks.append((pr.i, pr.j))
        if away:
            upd = run.iterate(k, pr, NAN, 0.0, 0.0, eps)
        else:
            u = _fw_decide(m, pr.w_i, pr.w_j, eps)[2]
            upd = None if u is None else (pr.i,) + u
        if upd is None:
            break
        dev.update(*upd)
    return picks


@pytest.mark.parametrize("m,n,start", N.RUN_SHAPES)
def test_whole_runs_on_axis_designs_are_bit_exact(acc, L, m, n, start):
    """D_opt_FW and D_opt_FW_away, 60 iterations with eps = -1 and the away variant with an eps that stops it (1.0),
    on designs whose trajectories take Frank-Wolfe and away steps: x, SP, SN, the final (x, w, H) and the sequence
    of (i, j) equal those of the float64 restatement bit for bit; F to 1e-12 (1 + |F|) (a Cholesky log-sum on the
    device, det in the oracle)."""
    from accbpg_and_fw_amd.D_opt_alg import _AwayRun, _fw_decide
    s, x0 = N.axis_run_design(m, n, start)
    dev, V, G = _axis_dev(L, m, n, s, x0)
    dev.close()
    obj = acc.DOptimalObj(V)
    lib = L.load()

    def state():
        x = torch.empty(n, dtype=torch.float64, device="cuda")
        w = torch.empty(n, dtype=torch.float64, device="cuda")
        H = torch.empty(m, m, dtype=torch.float64, device="cuda")
        assert lib.accbpg_fw_get_state(obj._h, C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()),
                                       C.c_void_p(H.data_ptr())) == L.OK
        return x.cpu().numpy(), w.cpu().numpy(), H.cpu().numpy()

    make_run = lambda m_, it: _AwayRun(m_, it, 0, 1)
    refs = {}
    for away, eps in ((0, -1.0), (1, -1.0), (1, 1.0)):
        ref = N.run_away(V, x0, eps, 60, make_run) if away else N.run_fw(V, x0, eps, 60, _fw_decide)
        refs[(away, eps)] = ref
        x, F, SP, SN, T = (acc.D_opt_FW_away if away else acc.D_opt_FW)(obj, x0, eps, 60, verbose=False)
        assert len(F) == len(ref[1]) == (60 if eps < 0 else len(ref[1])) and (eps < 0 or len(F) < 60)
        np.testing.assert_array_equal(x, ref[0])
        np.testing.assert_array_equal(SP, ref[2])
        np.testing.assert_array_equal(SN, ref[3])
        assert np.all(np.isfinite(ref[1]))
        assert np.max(np.abs(F - ref[1]) / (1 + np.abs(ref[1]))) <= 1e-12
        # the last iteration of a run that did not stop still applied its update: the reference's state has it too
        for got, want in zip(state(), ref[5]):
            np.testing.assert_array_equal(got, want)
    with Dev(L, V) as dev:
        for (away, eps), ref in refs.items():
            _axis_init(dev, m, n, s, x0, G)
            assert _drive(dev, m, away, eps, 60) == ref[4]
            for got, want in zip(dev.state(), ref[5]):
                np.testing.assert_array_equal(got, want)


# ----------------------------------------------------------------------------- c. one update on Gaussian data
# (520, 300): 64 row splits of 9 rows, splits 58 to 63 empty.  With m > n the Gram matrix V diag(x) V^T has rank at
# most n < m: no inverse H exists, so there is no Frank-Wolfe state to update.  That shape goes through the helpers
# (the same pass over V), and (520, 600) -- the same 64 splits of 9 rows -- carries the empty splits through the update.
UPDATE_SHAPES = [(8, 40, 40), (37, 203, 203), (37, 203, 204), (130, 1024, 1024), (256, 1024, 1024), (258, 777, 780),
                 (520, 300, 300), (520, 600, 600), (64, 4097, 4097)]
RATIOS = {}


def _ratio(name, err, bound):
    err, bound = np.asarray(err, dtype=np.longdouble), np.asarray(bound, dtype=np.longdouble)
    assert np.all(bound > 0)
    r = float(np.max(err / bound))
    RATIOS[name] = max(RATIOS.get(name, 0.0), r)
    print("ratio to bound  %-28s %.4f" % (name, r))
    return r


@pytest.mark.parametrize("m,n,ldv", UPDATE_SHAPES)
def test_one_update_on_gaussian_data_within_forward_bounds(L, m, n, ldv):
    from accbpg_and_fw_amd.D_opt_alg import _fw_decide
    V = gaussian_design(m, n, 1000 + m + ldv)
    tag = "(%d,%d,%d)" % (m, n, ldv)
    g = N.gamma
    with Dev(L, V, ldv) as dev:
        # the helpers
        for j in (0, n - 1, 2 * (n // 3) + 1):
            np.testing.assert_array_equal(dev.column(j), V[:, j])
        q = np.random.RandomState(m).randn(m)
        u = dev.vt_times(q)
        ql, Vl = q.astype(np.longdouble), V.astype(np.longdouble)
        assert _ratio("vt_times " + tag, np.abs(u - ql.dot(Vl)), g(m + 1) * np.abs(ql).dot(np.abs(Vl))) <= 1.0
        if m >= n:
            return
        # three genuine Frank-Wolfe steps, so that H is not fresh
        dev.init(np.ones(n) / n)
        for _ in range(3):
            pr = dev.probe(0)
            dev.update(pr.i, *_fw_decide(m, pr.w_i, pr.w_j, -1.0)[2])
        pr = dev.probe(0)
        genuine = (pr.i,) + _fw_decide(m, pr.w_i, pr.w_j, -1.0)[2]
        arbitrary = (n - 1, 0.7, -0.01, 0.3, 1.9)
        for name, (p, xscale, xadd, hcoef, hdiv) in (("genuine", genuine), ("arbitrary", arbitrary)):
            x, w, H = dev.state()
            dev.update(p, xscale, xadd, hcoef, hdiv)
            x1, w1, H1 = dev.state()
            q_prev = dev.probe(0).q_prev
            ref = N.update_ref(V, H, w, p, hcoef, hdiv)
            np.testing.assert_array_equal(x1, N.update_x(x, p, xscale, xadd))
            np.testing.assert_array_equal(H1, H1.T)
            assert np.all(np.isfinite(H1)) and np.all(np.isfinite(w1))
            bH = g(2 * m + 5) * (np.abs(H) + abs(hcoef) * np.outer(ref.A, ref.A)) / abs(hdiv)
            bw = g(4 * m + 5) * (np.abs(w) + abs(hcoef) * ref.B ** 2) / abs(hdiv)
            rH = _ratio("H' %s %s" % (name, tag), np.abs(H1 - ref.H), bH)
            rw = _ratio("w' %s %s" % (name, tag), np.abs(w1 - ref.w), bw)
            rq = _ratio("q  %s %s" % (name, tag), np.abs(q_prev - ref.q), g(2 * m + 1) * ref.Q)
            assert rH <= 1.0 and rw <= 1.0 and rq <= 1.0
            # (the update did something: against the pre-state the same distances are many bounds wide)
            assert np.max(np.abs(w1 - w) / bw) > 1e3 and np.max(np.abs(H1 - H) / bH) > 1e3


# --------------------------------------------------------------------------------------- d. lock-step wrappers
@pytest.mark.parametrize("n", [4097, 131072 + 257])
def test_lock_step_probe_equals_single_handle(acc, L, n):
    """K = 3 instances with a different plant each, mask [1, 0, 1]: every active record equals the single-handle one
    (and the restatement), fresh and from the fused stage-1 records of a lock-step update; the inactive record is
    untouched."""
    m, start = _shape(n)
    K = 3
    seams = _seams(n)
    plants = [(seams[q % len(seams)], seams[(q + 1) % len(seams)], kind) for q, kind in ((0, "tie"), (1, "twin"), (2, "tie"))]
    Vs, X0, designs = [], [], []
    for (a, b), (c, d), kind in plants:
        s, x0 = N.axis_base(m, n, start)
        s[a], s[b] = 2.0, (2.0 if kind == "tie" else 4.0)
        s[c], s[d] = 0.5, (0.5 if kind == "tie" else 0.25)
        G = np.array(N.axis_exact(m, s, x0))
        Vs.append(N.axis_design(m, n, s, x0)[0]); X0.append(x0); designs.append((s, G))
    batch = acc.DOptimalBatch(Vs)
    lib = L.load()
    batch.fw_init(torch.from_numpy(np.stack(X0)).cuda())
    for i, ((a, b), (c, d), kind) in enumerate(plants):
        x, w, H = [t.cpu().numpy() for t in batch.fw_state(i)]
        s, G = designs[i]
        np.testing.assert_array_equal(H, np.diag(1.0 / G))
        np.testing.assert_array_equal(w, s * s / G[np.arange(n) % m])
        hi = batch.instance(i)._h
        for t, (p, cval) in enumerate([(c, 0.125), (d, 0.125), (start + 1, 0.25), (start + 4 * m - 1, 0.0625)]):
            assert lib.accbpg_fw_update(hi, p, 0.0 if t == 0 else 1.0, cval, 0.0, 1.0) == L.OK
    mask = (C.c_int * K)(1, 0, 1)
    noop = [NOOP] * K
    for away in (0, 1):
        exp = []
        for i in range(K):
            x, w, _ = [t.cpu().numpy() for t in batch.fw_state(i)]
            exp.append(N.probe(w, x, away))
            (a, b), (c, d), kind = plants[i]
            assert (exp[i].i, exp[i].j) == ((a, c) if kind == "tie" else (b, d))
        for how in ("as it comes", "fresh", "fused stage 1"):
            if how == "fused stage 1":
                batch.fw_update([True, False, True], noop)
            probes = (L.FwProbe * K)()
            for i in range(K):
                probes[i].i, probes[i].j, probes[i].w_i, probes[i].w_j, probes[i].x_j = -7, -7, -7.0, -7.0, -7.0
            assert lib.accbpg_dopt_batch_fw_probe(batch._h, away, mask, probes) == L.OK
            assert (probes[1].i, probes[1].j, probes[1].w_i, probes[1].w_j, probes[1].x_j) == (-7, -7, -7.0, -7.0, -7.0)
            for i in (0, 2):
                _rec_equal(probes[i], exp[i], (n, away, how, i))
        for i in (0, 2):                                                  # the single-handle record of the same state
            one = L.FwProbe()
            assert lib.accbpg_fw_probe_step(batch.instance(i)._h, away, 0, C.byref(one)) == L.OK
            _rec_equal(one, exp[i], (n, away, "single handle", i))
    x1 = batch.fw_state(1)[0].cpu().numpy()                               # the inactive instance's state: untouched
    (a, b), (c, d), kind = plants[1]
    e = np.zeros(n); e[c] = 0.125; e[d] = 0.125; e[start + 1] = 0.25; e[start + 4 * m - 1] = 0.0625
    np.testing.assert_array_equal(x1, e)
