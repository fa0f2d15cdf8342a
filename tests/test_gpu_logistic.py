"""GPU tests of the logistic family: LogisticRegression (logistic_kernels.hip) and L2L1Linf (vec_kernels.hip) on the
device against the float64 restatement, the np.longdouble reference and the forward bounds of tests/logistic_numpy.py,
and against the goldens of the real reference (tests/golden/logistic.npz).

Exact data (A integers in [-4, 4], x multiples of 1/64, y = +-1): A x is exact in any summation order, so fitted() must
equal NumPy's product in every launch form (same_values: only a zero's sign may differ, see there), and every
device-against-device comparison -- flags, call forms, strides, repeats -- is bit for bit (same_bits); losses() and
weights() are held entry by entry to T_ULP and Q_ULP ulps of the
np.longdouble values; the sum of t must be bit-equal to reduce_numpy.tree_sum of the device's own losses(), which pins
the reduction apart from the math library; f and g lie inside their forward bounds.  The shapes are those of
tests/test_gpu_svm.py (the launch forms and their selecting conditions are the same; test_logistic_cpu.py checks the
reach of the list):

  pass 1, a wavefront per row          (1,1) (3,2) (4,64) (5,65) (7,129) (2050,130) (416,1540)
  pass 1, a workgroup per row          (33,4096) (5,4097)
  pass 1, wavefront with the LDS hold  (2048,32768)
  16-byte / scalar loads               even lda and A, x on 16 bytes / odd lda, x carved at 8 mod 16; odd n: the tail
  pass 2, vt_nsplit 1 / between / m/8 cap / 64 cap, as in test_gpu_svm.py

Planted rows put s = y*(A x) at 0, -0.0, +-36, +-37, +-50, +-700, +-745, +-746, +-1e4, +-inf and NaN exactly.  Whole
runs against the goldens: the same length, F to 1e-9, x within the reference's own spread + 1e-9, G to 1e-9 relative,
the printed column to 1e-12."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logistic_numpy as LN  # noqa: E402
import reduce_numpy as T  # noqa: E402
from conftest import golden  # noqa: E402

pytestmark = pytest.mark.gpu
LD = LN.LD


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def gold():
    return golden("logistic")


def same_bits(a, b):
    """bit for bit as float64, the sign of a zero included; every NaN counts as the same NaN"""
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64)).copy()
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64)).copy()
    a[np.isnan(a)], b[np.isnan(b)] = np.nan, np.nan
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_values(a, b):
    """Equal as float64 values, a NaN equal to a NaN, -0.0 equal to +0.0: for the device's exact A x against a host
    product.  A row whose products are all -0.0 sums to -0.0 in NumPy, while the device's fma chain starts at +0.0 and
    stays there; every other value of an exact sum has one bit pattern."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def on_device(A, lda_pad, x, x_skew):
    """A in a (m, n + lda_pad) device matrix whose gap columns hold NaN, x at 16 bytes or at 8 mod 16"""
    m, n = A.shape
    big = torch.full((m, n + lda_pad), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :n] = torch.from_numpy(A)
    Ad = big[:, :n]
    xb = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    off = ((1 if x_skew else 0) - xb.data_ptr() // 8) % 2
    xd = xb[off:off + n]
    xd.copy_(torch.from_numpy(x))
    assert xd.data_ptr() % 16 == (8 if x_skew else 0) and Ad.stride(0) == n + lda_pad
    return Ad, xd


def evaluate(acc, A, x, y, lda_pad=0, x_skew=False):
    """one func_grad(x, 2) -> dict(f, g, z, t, r, obj, xd)"""
    Ad, xd = on_device(A, lda_pad, x, x_skew)
    f = acc.LogisticRegression(Ad, torch.from_numpy(y).cuda())
    v, g = f.func_grad(xd, 2)
    return dict(f=v, g=g.cpu().numpy(), z=f.fitted(), t=f.losses(), r=f.weights(), obj=f, xd=xd)


def check_exact(acc, A, x, y, lda_pad=0, x_skew=False, tag=""):
    m, n = A.shape
    d = evaluate(acc, A, x, y, lda_pad, x_skew)
    z = A.dot(x)
    assert same_values(d["z"], z)
    ref = LN.refs_and_bounds(A, z, y)
    et, er = np.abs(LD(d["t"]) - ref["t"]), np.abs(LD(d["r"]) - ref["r"])
    ef, eg = abs(LD(d["f"]) - ref["f"]), np.abs(LD(d["g"]) - ref["g"])
    live = ref["g_bound"] > 0                                   # (a column of zeros has g = 0 and the bound 0)
    print("%s(%d,%d): t %.3f of its bound, r %.3f, f %.3f, g %.3f" % (
        tag, m, n, float(np.max(et / ref["t_bound"])), float(np.max(er / ref["r_bound"])), float(ef / ref["f_bound"]),
        float(np.max(eg[live] / ref["g_bound"][live])) if live.any() else 0.0))
    assert np.all(et <= ref["t_bound"])
    assert np.all(er <= ref["r_bound"])
    # the reduction alone: the device's own terms on the emulated tree
    assert same_bits(d["f"], T.tree_sum(d["t"], T.CAP_VEC) / m)
    assert ef <= ref["f_bound"]
    assert np.all(eg <= ref["g_bound"])
    return d


@pytest.mark.parametrize("m,n", LN.EXACT_SHAPES)
def test_exact_data_every_launch_form(acc, m, n):
    A, x, y = LN.exact_data(m, n, 100 * m + n)
    d = check_exact(acc, A, x, y)
    f, xd = d["obj"], d["xd"]
    # flags 0 / 1 / 2 agree bit for bit, and so do the call forms
    assert same_bits(f.func_grad(xd, 0), d["f"]) and same_bits(f(xd), d["f"]) and same_bits(f.f(xd), d["f"])
    assert same_bits(f.func_grad(xd, 1).cpu().numpy(), d["g"]) and same_bits(f.gradient(xd).cpu().numpy(), d["g"])
    vn, gn = f.func_grad(np.ascontiguousarray(xd.cpu().numpy()), 2)                 # NumPy in, NumPy out
    assert isinstance(gn, np.ndarray) and same_bits(vn, d["f"]) and same_bits(gn, d["g"])
    assert same_bits(f.fitted(), d["z"]) and same_bits(f.losses(), d["t"]) and same_bits(f.weights(), d["r"])


def test_launch_forms_are_all_reached(acc):
    """the shapes above and (2048,32768) cover every selecting condition on this device"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = LN.all_shapes()
    wg_row = [s for s in shapes if LN.ax_form(s[0], s[1], cu) == "wg"]
    wave_row = [s for s in shapes if LN.ax_form(s[0], s[1], cu) != "wg"]
    assert (33, 4096) in wg_row and (5, 4097) in wg_row
    assert any(m >= 8 * cu for m, n in wave_row) and any(n < 4096 and m < 8 * cu for m, n in wave_row)
    splits = {s: LN.vt_nsplit(s[0], s[1], cu) for s in shapes}
    assert any(v == 1 for v in splits.values())
    assert any(v == s[0] // 8 and 1 < v < 64 for s, v in splits.items()), splits
    assert any(1 < v < min(64, s[0] // 8) for s, v in splits.items()), splits
    if cu <= 256:
        assert any(LN.ax_form(m, n, cu) == "hold" for m, n in shapes)


@pytest.mark.parametrize("m,n,pad,skew", [(5, 65, 2, False), (5, 65, 1, False), (7, 129, 3, False), (7, 129, 0, True),
                                          (4, 64, 6, True), (5, 4097, 1, False), (33, 4096, 5, False),
                                          (33, 4096, 0, True), (2050, 130, 2, True)])
def test_exact_data_strides_and_alignment(acc, m, n, pad, skew):
    """an even lda > n (16-byte loads, odd n: the one-column tail), an odd lda > n (scalar loads), an x carved at 8 mod
    16: the same bits as the aligned call on the same data (A x is exact, so the epilogue sees the same z, and pass 2
    does not depend on the loads of pass 1); the gap columns hold NaN and must not be read"""
    A, x, y = LN.exact_data(m, n, 7 * m + n + pad)
    d = check_exact(acc, A, x, y, lda_pad=pad, x_skew=skew, tag="pad %d skew %d " % (pad, skew))
    a = evaluate(acc, A, x, y)
    for k in ("f", "z", "t", "r"):
        assert same_bits(d[k], a[k]), k
    # pass 2 takes 16-byte loads or scalar loads by lda: its sums run in the same order either way
    assert same_bits(d["g"], a["g"])


def test_exact_data_long_rows_with_lds_hold(acc):
    """(2048,32768): a wavefront per row held to two workgroups per CU by its LDS request.  The data is drawn on the
    device (small integers, 0.5 GB); the row references come from the device's exact A x."""
    m, n = LN.LONG_SHAPE
    gen = torch.Generator(device="cuda").manual_seed(5)
    A = torch.randint(-4, 5, (m, n), generator=gen, device="cuda").to(torch.float64)
    x = torch.randint(-256, 257, (n,), generator=gen, device="cuda").to(torch.float64) / 64.0
    # margins of every size: scale the rows so that |s| spreads from below 1 to the thousands
    x = x * (torch.arange(n, device="cuda") < 64).to(torch.float64)
    y = torch.randint(0, 2, (m,), generator=gen, device="cuda").to(torch.float64) * 2 - 1
    z = (A[:, :64] @ x[:64]).cpu().numpy()                      # exact: 64 products of small integers
    f = acc.LogisticRegression(A, y)
    v, g = f.func_grad(x, 2)
    yh = y.cpu().numpy()
    assert same_values(f.fitted(), z)
    t, r = f.losses(), f.weights()
    tr, rr = LN.row_refs(z, yh)
    assert np.all(np.abs(LD(t) - tr) <= LN.ulps(LN.T_ULP, tr)) and np.all(np.abs(LD(r) - rr) <= LN.ulps(LN.Q_ULP, rr))
    assert same_bits(v, T.tree_sum(t, T.CAP_VEC) / m) and same_bits(f.func_grad(x, 0), v)
    fb = (np.sum(LN.ulps(LN.T_ULP, tr)) + LN.gamma(T.tree_depth(m, T.CAP_VEC)) * np.sum(tr)) / m + LN.U * np.sum(tr) / m
    assert abs(LD(v) - np.sum(tr) / m) <= fb
    # the gradient against a float64 product on the device with the device's own r: A is exact, so the two differ by
    # the rounding of two summation orders, each at most gamma_(m+64) of sum |A||r|
    rd = torch.from_numpy(r).cuda()
    gref = (rd @ A) / m
    bound = (2 * LN.gamma(m + 64) * (rd.abs() @ A.abs()) / m + 2 * LN.U * gref.abs()).cpu().numpy()
    assert np.all(np.abs(g.cpu().numpy() - gref.cpu().numpy()) <= bound)
    assert same_bits(f.func_grad(x, 1).cpu().numpy(), g.cpu().numpy())


@pytest.mark.parametrize("m,n", LN.PLANTED_SHAPES)
def test_planted_margins(acc, m, n):
    A, x, y, s = LN.planted(m, n, 3)
    d = evaluate(acc, A, x, y)
    with np.errstate(invalid="ignore"):
        z = A.dot(x)
        assert same_values(d["z"], z) and same_bits((y * d["z"])[:s.size], s)
    t, r = d["t"], d["r"]
    for i, si in enumerate(s):
        yi = y[i]
        if np.isnan(si):
            assert np.isnan(t[i]) and np.isnan(r[i])
        elif si == np.inf:
            assert t[i] == 0.0 and np.isnan(r[i])               # q = 0, r = -(inf*0)
        elif si == -np.inf:
            assert t[i] == np.inf and r[i] == np.inf            # q = 1, r = -(-inf*1)
        elif si >= 746:
            assert t[i] == 0.0 and r[i] == 0.0 and np.signbit(r[i]) == np.signbit(-0.0 * yi)
        elif si <= -746:
            assert t[i] == -si and r[i] == -yi
        elif si == 0:
            tr, _ = LN.tq_ref(np.array([0.0]))
            assert abs(LD(t[i]) - tr[0]) <= LN.ulps(LN.T_ULP, tr[0]) and r[i] == -yi / 2
        else:
            tr, qr = LN.tq_ref(np.array([si]))
            assert abs(LD(t[i]) - tr[0]) <= LN.ulps(LN.T_ULP, tr[0]), (si, t[i])
            assert abs(LD(r[i]) + yi * qr[0]) <= LN.ulps(LN.Q_ULP, qr[0]), (si, r[i])
    # the rows that were not planted stay inside the row bounds
    k = s.size
    if k < m:
        tr, rr = LN.row_refs(z[k:], y[k:])
        assert np.all(np.abs(LD(t[k:]) - tr) <= LN.ulps(LN.T_ULP, tr))
        assert np.all(np.abs(LD(r[k:]) - rr) <= LN.ulps(LN.Q_ULP, rr))
    # NaN rows give a NaN value and NaN in every column: the planted rows are zero outside column 0, and 0*NaN of a
    # row with A_ij = 0 still reaches g_j
    assert np.count_nonzero(A[:s.size, 1:]) == 0
    assert np.isnan(d["f"]) and np.all(np.isnan(d["g"]))
    # without the non-finite rows the value and the gradient are finite and inside their bounds
    keep = np.isfinite(y)
    check_exact(acc, A[keep], x, y[keep], tag="planted, finite rows ")


def test_nan_reaches_only_the_columns_it_should(acc):
    """a NaN entry of A: its row's t and r are NaN, f is NaN, and g is NaN in every column (r_i = NaN multiplies every
    A_ij of the row, zeros included); a NaN in x makes everything NaN"""
    A, x, y = LN.exact_data(33, 130, 12)
    A[5, 7] = np.nan
    A[5, 9] = 0.0
    d = evaluate(acc, A, x, y)
    assert np.isnan(d["f"]) and np.isnan(d["t"][5]) and np.isnan(d["r"][5]) and np.isnan(d["z"][5])
    assert np.isnan(d["t"]).sum() == 1 and np.all(np.isnan(d["g"]))
    A, x, y = LN.exact_data(33, 130, 13)
    x[3] = np.nan
    d = evaluate(acc, A, x, y)
    assert np.isnan(d["f"]) and np.all(np.isnan(d["g"]))


def test_calls_repeat_and_arguments_are_checked(acc):
    rng = np.random.RandomState(2)
    for m, n in [(96, 40), (33, 4100), (2050, 131)]:
        A, x = rng.randn(m, n), rng.randn(n) * 0.1
        y = rng.choice([-1.0, 1.0], size=m)
        f = acc.LogisticRegression(A, y, alpha=0.5)
        assert f.X is A and f.y is y and f.alpha == 0.5 and (f.m, f.n) == (m, n)
        v1, g1 = f.func_grad(x, 2)
        rows1 = (f.fitted(), f.losses(), f.weights())
        v2, g2 = f.func_grad(x, 2)
        assert same_bits(v1, v2) and same_bits(g1, g2)
        assert all(same_bits(a, b) for a, b in zip(rows1, (f.fitted(), f.losses(), f.weights())))
        assert same_bits(f.func_grad(x, 1), g1) and same_bits(f.func_grad(x, 0), v1)
    with pytest.raises(AssertionError):
        f.func_grad(np.zeros(5), 2)
    with pytest.raises(AssertionError):
        f.func_grad(x, 3)
    # labels of any real value, and an (m, 1) column as the example draws it
    A, x, y = LN.exact_data(33, 130, 4)
    y2 = y * np.random.RandomState(1).choice([0.5, 1.0, 2.0], size=33)
    d = acc.LogisticRegression(A, y2.reshape(-1, 1))
    v, g = d.func_grad(x, 2)
    ref = LN.refs_and_bounds(A, A.dot(x), y2)
    assert abs(LD(v) - ref["f"]) <= ref["f_bound"]
    yq = LN.U * np.abs(ref["r"]).dot(np.abs(A)) / 33                                # y*q rounds
    assert np.all(np.abs(LD(g) - ref["g"]) <= ref["g_bound"] + yq)


# -------------------------------------------------------------------------------------------------------- goldens
def gauss(gold):
    A, y = LN.gaussian_instance()
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["gauss_A_checksum"], rtol=1e-14)
    return A, y


def test_general_data_golden_points(acc, gold):
    """The device against the np.longdouble reference inside the general-data bounds; the golden (a float64 NumPy
    evaluation that lies inside the bounds with a dot product's chain length, test_logistic_cpu.py) then differs from
    the device by at most the sum of the two bounds."""
    A, y = gauss(gold)
    f = acc.LogisticRegression(A, y)
    for i, x in enumerate(gold["pc_x"]):
        v, g = f.func_grad(x, 2)
        z = f.fitted()
        zl = np.asarray(A, dtype=LD).dot(np.asarray(x, dtype=LD))
        ds = LN.ds_bound(A, x, y, y * z)
        assert np.all(np.abs(LD(z) - zl) <= ds)
        ref = LN.refs_and_bounds(A, zl.astype(np.float64), y, ds=ds + LN.U * np.abs(zl))
        df, dg = abs(LD(v) - ref["f"]), np.abs(LD(g) - ref["g"])
        print("point %d: |df| %.2e (bound %.2e)  max |dg|/bound %.3f" % (i, float(df), float(ref["f_bound"]),
                                                                          float(np.max(dg / ref["g_bound"]))))
        assert df <= ref["f_bound"] and np.all(dg <= ref["g_bound"])
        assert np.all(np.abs(LD(f.losses()) - ref["t"]) <= ref["t_bound"])
        assert np.all(np.abs(LD(f.weights()) - ref["r"]) <= ref["r_bound"])
        dsn = LN.ds_bound(A, x, y, y * z, chain=A.shape[1])     # the goldens: a NumPy dot product
        refn = LN.refs_and_bounds(A, zl.astype(np.float64), y, ds=dsn + LN.U * np.abs(zl))
        assert abs(v - gold["pc_f"][i]) <= ref["f_bound"] + refn["f_bound"]
        assert np.all(np.abs(g - gold["pc_g"][i]) <= ref["g_bound"] + refn["g_bound"])
        assert np.all(np.abs(z - gold["pc_Ax"][i]) <= ds + dsn)
        assert same_bits(f.func_grad(x, 1), g) and same_bits(f.func_grad(x, 0), v)


def printed(text, col=2):
    rows = [ln.split() for ln in text.splitlines() if ln[:6].strip().isdigit()]
    return np.array([float(r[col]) for r in rows])


RUN_NAMES = list(LN.run_table(LN.SOLVERS, LN.lmo_linf_ball))


@pytest.fixture(scope="module")
def run_problem(acc, gold):
    """the factory at the example's shape with the stored mixed labels"""
    m, n, seed = LN.EXAMPLE["m"], LN.EXAMPLE["n"], LN.EXAMPLE["seed"]
    f, h, L, x0 = acc.Logistic_regr_L2L1Linf(m, n, randseed=seed, labels=gold["run_y"])
    A = f.X
    np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["run_A_checksum"], rtol=1e-14)
    assert L == float(gold["run_L"]) and h.lamda == float(gold["run_lamda"]) and h.B == float(gold["run_B"])
    return f, h, L, x0


@pytest.mark.parametrize("name", RUN_NAMES)
def test_whole_runs_against_goldens(acc, gold, run_problem, name):
    f, h, L, x0 = run_problem
    key = "run_" + name
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        x, F, G = LN.run_table(acc, acc.lmo_linf_ball)[name](f, h, acc.SquaredL2Norm(), L, np.copy(x0), h.B)
    Fr, Gr = gold[key + "_F"], gold[key + "_G"]
    assert int(gold[key + "_prefix"]) == len(Fr)
    assert len(F) == len(Fr)
    dF = np.abs(F - Fr) / (1 + np.abs(Fr))
    dx = float(np.max(np.abs(x - gold[key + "_x"])))
    print("%s: len %d  max dF %.2e  dx %.2e (spread %.2e)" % (key, len(F), dF.max(), dx, float(gold[key + "_xspread"])))
    assert np.all(dF <= 1e-9)
    assert dx <= float(gold[key + "_xspread"]) + 1e-9
    np.testing.assert_allclose(G, Gr, rtol=1e-9)
    np.testing.assert_allclose(printed(buf.getvalue()), gold[key + "_Lk"], rtol=1e-12)


def test_descent_step_frank_wolfe_runs_on_the_objective(acc, run_problem):
    f, h, L, x0 = run_problem
    with contextlib.redirect_stdout(io.StringIO()):
        x, F = acc.FW_alg_descent_step(f, acc.SquaredL2Norm(), np.copy(x0), 30, lmo=acc.lmo_linf_ball(h.B))[:2]
    assert np.all(np.isfinite(F)) and F[-1] < F[0] and np.max(np.abs(x)) <= h.B


def test_factory_draws_are_the_examples(acc):
    np.random.seed(5)
    f, h, L, x0 = acc.Logistic_regr_L2L1Linf(12, 7)
    after = np.random.random_sample()
    A, b = LN.example_draws(12, 7, seed=5)
    assert np.random.random_sample() == after                   # the generator stands where the example leaves it
    assert same_bits(f.X, A) and same_bits(f.y, b.reshape(-1)) and np.all(f.y == 1.0)
    assert h.lamda == 1.0 / 12 and h.B == 1 and L == 0.25 and same_bits(x0, np.zeros(7)) and isinstance(h, acc.L2L1Linf)
    f2, h2, _, _ = acc.Logistic_regr_L2L1Linf(12, 7, lamda=0.3, B=2.5, randseed=5, labels=-np.ones(12))
    assert np.random.random_sample() == after and same_bits(f2.X, A) and np.all(f2.y == -1.0)
    assert h2.lamda == 0.3 and h2.B == 2.5
    ref = LN.refs_and_bounds(A, A.dot(np.full(7, 0.25)), -np.ones(12),
                             ds=LN.ds_bound(A, np.full(7, 0.25), -np.ones(12), A.dot(np.full(7, 0.25))))
    assert abs(LD(f2(np.full(7, 0.25))) - ref["f"]) <= ref["f_bound"]


# ------------------------------------------------------------------------------------------------------- L2L1Linf
def prox_inputs(n, L, lamda, B):
    """(y, g) with planted entries: |v| == thr exactly, v == +-B, NaN, +-inf, zeros of both signs"""
    y, g = T.draw(n, 1) * 0.5, T.draw(n, 2)
    thr = lamda / L
    plant = [(-thr) * L, thr * L, -B * L, B * L, np.nan, np.inf, -np.inf, 0.0, -0.0, (-(B + thr)) * L, (B + thr) * L]
    for i, v in enumerate(plant[:n]):
        g[i], y[i] = v, 0.0                         # v = -((1/L)*g): +-thr and +-B exactly when L is a power of two
    return y, g


@pytest.mark.parametrize("n", T.edge_sizes(T.CAP_VEC))
def test_l2l1linf_prox_maps_bit_for_bit(acc, n):
    for L, lamda, B in ((0.5, 0.25, 1.0), (4.0, 0.0, 0.75), (0.05, 1.0 / 96, 1.0)):
        h, hr = acc.L2L1Linf(lamda=lamda, B=B), LN.L2L1Linf(lamda=lamda, B=B)
        y, g = prox_inputs(n, L, lamda, B)
        yd, gd = torch.from_numpy(y).cuda(), torch.from_numpy(g).cuda()
        for got, want in ((h.prox_map(gd, L), hr.prox_map(g, L)),
                          (h.div_prox_map(yd, gd, L), hr.div_prox_map(y, g, L))):
            got = got.cpu().numpy()
            assert same_bits(got, want)
            assert np.array_equal(np.signbit(got[want == 0]), np.signbit(want[want == 0]))     # |v| <= thr -> +0.0
        if n >= 11 and L in (0.5, 4.0):
            p = h.prox_map(gd, L).cpu().numpy()
            thr = lamda / L
            # v = +thr, -thr -> 0; v = +B, -B -> +-(B - thr); NaN kept; -+inf -> +-B; +-(B + thr) -> +-B exactly
            assert p[0] == 0 and p[1] == 0 and p[2] == B - thr and p[3] == -(B - thr) and np.isnan(p[4])
            assert p[5] == -B and p[6] == B and p[7] == 0 and p[8] == 0 and p[9] == B and p[10] == -B
        # NumPy in, NumPy out; lamda and B are read at every call
        out = h.div_prox_map(y, g, L)
        assert isinstance(out, np.ndarray) and same_bits(out, hr.div_prox_map(y, g, L))
    h.lamda, h.B = 0.3, 0.5
    assert same_bits(h.prox_map(g, L), LN.L2L1Linf(0.3, 0.5).prox_map(g, L))
    with pytest.raises(AssertionError):
        h.prox_map(g, 0.0)


@pytest.mark.parametrize("n", T.edge_sizes(T.CAP_VEC))
def test_l2l1linf_sums_on_the_fixed_tree(acc, n):
    from accbpg_and_fw_amd.algorithms import _divergences
    h, hr = acc.L2L1Linf(lamda=0.3, B=1.0), LN.L2L1Linf(lamda=0.3, B=1.0)
    g, x, y, z, z1 = (T.draw(n, k) for k in (3, 4, 5, 6, 7))
    gd, xd, yd, zd, z1d = (torch.from_numpy(v).cuda() for v in (g, x, y, z, z1))
    assert same_bits(h.extra_Psi(xd), 0.3 * T.tree_sum(np.abs(x), T.CAP_VEC))
    assert same_bits(h(xd), 0.5 * T.tree_sum(x * x, T.CAP_VEC))
    e_lin, e_xy, e_zz = hr.ls_elementwise(g, x, y, z, z1)
    want = (T.tree_sum(e_lin, T.CAP_VEC), 0.5 * T.tree_sum(e_xy, T.CAP_VEC), 0.5 * T.tree_sum(e_zz, T.CAP_VEC))
    got = h.ls_terms(gd, xd, yd, zd, z1d)
    assert all(same_bits(a, b) for a, b in zip(got, want)), (got, want)
    assert _divergences(h, gd, xd, yd, zd, z1d) == got
    # terms that are not wanted
    assert h.ls_terms(None, xd, yd) == (0.0, want[1], 0.0) and h.ls_terms(gd, xd, yd)[:2] == want[:2]
    assert same_bits(h.divergence(xd, yd), want[1]) and same_bits(h.divergence(x, y), want[1])
    assert h.gradient(xd) is xd
    if n <= 4096:
        x[0] = np.nan
        assert np.isnan(h.extra_Psi(x)) and np.isnan(h.ls_terms(g, x, y)[1])


def test_l2l1linf_golden_values(acc, gold):
    """the device's prox maps have the reference's bits; its sums lie within the rounding of two summation orders"""
    A, _ = gauss(gold)
    pts, n = gold["pc_x"], A.shape[1]
    for a, lamda in enumerate(gold["k_lamda"]):
        h = acc.L2L1Linf(lamda=float(lamda), B=1)
        for i, x in enumerate(pts):
            g = gold["pc_g"][i]
            for b, L in enumerate(gold["k_L"]):
                assert same_bits(h.prox_map(g, float(L)), gold["k_prox"][a, b, i])
                assert same_bits(h.div_prox_map(x, g, float(L)), gold["k_dprox"][a, b, i])
            tol = 2 * LN.gamma(n + 32)
            assert abs(h.extra_Psi(x) - gold["k_psi"][a, i]) <= tol * abs(gold["k_psi"][a, i])
            assert abs(h.divergence(x, pts[(i + 1) % 3]) - gold["k_div"][i]) <= tol * gold["k_div"][i]
            assert abs(h(x) - gold["k_h"][i]) <= tol * gold["k_h"][i]
