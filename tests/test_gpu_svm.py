"""GPU tests of the SVM family: SVM_fun (svm_kernels.hip) and PolyDiv on the device against the NumPy formulas, the
restatement (tests/svm_numpy.py) and the goldens of the real reference (tests/golden/svm.npz).

Exact data.  A holds integers in [-8, 8], x multiples of 1/64 in [-4, 4], y is +-1 (or a power-of-two multiple where
said): every product and every sum is exact in float64 whatever its order, so f, hinge_loss, g, subgradient_loss and
margins() must have the bits of the NumPy formulas for any lamda.  The shapes are the smallest that reach every launch
form of the new file (CU = compute units of the device, 256 on MI355X):

  pass 1, svm_ax_kernel<64> (a wavefront per row)        m >= 8*CU or n < 4096: (1,1) (3,2) (4,64) (5,65) (7,129)
                                                          (2050,130) [m >= 8*CU] (416,1540)
  pass 1, svm_ax_kernel<256> (a workgroup per row)       m < 8*CU and n >= 4096: (33,4096) (5,4097)
  pass 1, wavefront per row with the LDS hold            n >= 32768 (and m >= 8*CU): (2048,32768)
  16-byte loads / scalar loads                           even lda and A, x on 16 bytes / odd lda (5,65,+2 -> lda 67),
                                                          an x carved at 8 mod 16; odd n with 16-byte loads takes the
                                                          one-column tail: (5,65) at lda 66, (5,4097) at lda 4098
  sums: one block / several blocks of either vector      m, n <= 1024 / n = 4096, 4097, m = 2050
  pass 2, vt_nsplit = 1 / between / m/8 cap / 64 cap     (1,1) (3,2) (4,64) (5,65) (7,129) [m/8 = 0 -> 1]; (416,1540)
                                                          and (2048,32768) [between]; (33,4096) [m/8]; (2050,130) [64]
  gradient combine: one trip                             every shape (n < 2048*256)

General data: the golden per-call points, all margins at least 1e-6 from 1.  The indicator set must be the
reference's; f and g are held to forward bounds computed here from the data (gamma_k = k*u/(1 - k*u), u = 2^-53):
  |f - f_ref|   <= gamma_n*mean(|A||x|) + gamma_m*hinge + gamma_n*(lamda/2)<x,x>
  |g - g_ref|_j <= gamma_m*(|A|^T|r|)_j/m + 3u*(|lamda x_j| + |s_j/m|).

PolyDiv on the device against the restatement: 1e-13 relative (vectors: of the largest entry); whole runs against the
goldens: the same length, F to 1e-9, x within the reference's own spread + 1e-9, the printed L column to 1e-12."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_numpy as T  # noqa: E402
import svm_numpy as SN  # noqa: E402
from conftest import golden  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -53


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def gold():
    return golden("svm")


def gamma(k):
    return k * U / (1 - k * U)


def same_bits(a, b):
    """equal as float64 values, a NaN equal to a NaN (the sign of a zero is not compared: NumPy's 0*y*A terms may be
    -0.0 where the device adds +0.0 products)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def exact_data(m, n, seed, ymode="pm1"):
    rng = np.random.RandomState(seed)
    A = rng.randint(-8, 9, size=(m, n)).astype(np.float64)
    x = rng.randint(-256, 257, size=n) / 64.0
    if ymode == "pm1":
        y = rng.choice([-1.0, 1.0], size=m)
    else:
        y = rng.choice([-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0], size=m)
    return A, x, y


def numpy_all(lamda, A, x, y):
    """(F, hinge, g, subgradient, A x) by the NumPy formulas of the reference"""
    f = SN.SVM_fun(lamda, A, y)
    with np.errstate(invalid="ignore"):
        return f.F(x), f.hinge_loss(x), f.func_grad(x, 1), f.subgradient_loss(x), f.margins(x)


def vt_nsplit(m, n, cu):
    cb = (n + 511) // 512
    s = (4 * cu // 5 + cb // 2) // cb
    return max(1, min(s, 64, m // 8))


def on_device(A, lda_pad, x, x_skew):
    """A in a (m, n + lda_pad) device matrix, x at 16 bytes or at 8 mod 16"""
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


def check_exact(acc, A, x, y, lamda, lda_pad=0, x_skew=False):
    Ad, xd = on_device(A, lda_pad, x, x_skew)
    f = acc.SVM_fun(lamda, Ad, torch.from_numpy(y).cuda())
    F, hinge, g, sub, z = numpy_all(lamda, A, x, y)
    v2, g2 = f.func_grad(xd, 2)
    assert same_bits(f.margins(), z)
    assert same_bits(v2, F), (v2, F)
    assert same_bits(g2.cpu().numpy(), g)
    assert same_bits(f.func_grad(xd, 0), F) and same_bits(f(xd), F) and same_bits(f.F(xd), F)
    assert same_bits(f.func_grad(xd, 1).cpu().numpy(), g) and same_bits(f.gradient(xd).cpu().numpy(), g)
    assert same_bits(f.hinge_loss(xd), hinge)
    assert same_bits(f.subgradient_loss(xd).cpu().numpy(), sub)
    # NumPy in, NumPy out
    vn, gn = f.func_grad(np.ascontiguousarray(xd.cpu().numpy()), 2)
    assert isinstance(gn, np.ndarray) and same_bits(vn, F) and same_bits(gn, g)
    return f


EXACT_SHAPES = [(1, 1), (3, 2), (4, 64), (5, 65), (7, 129), (33, 4096), (5, 4097), (2050, 130), (416, 1540)]


@pytest.mark.parametrize("lamda", [0.0, 0.37])
@pytest.mark.parametrize("m,n", EXACT_SHAPES)
def test_exact_data_every_launch_form(acc, m, n, lamda):
    A, x, y = exact_data(m, n, 100 * m + n)
    check_exact(acc, A, x, y, lamda)


def test_launch_forms_are_all_reached(acc):
    """the shapes above and (2048,32768) cover every selecting condition on this device"""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    shapes = EXACT_SHAPES + [(2048, 32768)]
    wg_row = [s for s in shapes if s[0] < 8 * cu and s[1] >= 4096]
    wave_row = [s for s in shapes if not (s[0] < 8 * cu and s[1] >= 4096)]
    assert (33, 4096) in wg_row and (5, 4097) in wg_row
    assert any(m >= 8 * cu for m, n in wave_row) and any(n < 4096 and m < 8 * cu for m, n in wave_row)
    splits = {s: vt_nsplit(s[0], s[1], cu) for s in shapes}
    assert any(v == 1 for v in splits.values())
    assert any(v == s[0] // 8 and 1 < v < 64 for s, v in splits.items()), splits          # the m/8 cap
    assert any(1 < v < min(64, s[0] // 8) for s, v in splits.items()), splits             # in between
    if cu <= 256:
        assert any(m >= 8 * cu and n >= 32768 for m, n in shapes)                           # the LDS hold


@pytest.mark.parametrize("m,n,pad,skew", [(5, 65, 2, False), (5, 65, 1, False), (7, 129, 3, False), (7, 129, 0, True),
                                          (4, 64, 6, True), (5, 4097, 1, False), (33, 4096, 5, False),
                                          (33, 4096, 0, True), (2050, 130, 2, True)])
def test_exact_data_strides_and_alignment(acc, m, n, pad, skew):
    """an even lda > n (16-byte loads, odd n: the one-column tail), an odd lda > n (scalar loads), an x carved at 8 mod
    16 (scalar loads of pass 1, 16-byte loads of pass 2); the gap columns hold NaN and must not be read"""
    A, x, y = exact_data(m, n, 7 * m + n + pad)
    check_exact(acc, A, x, y, 0.25, lda_pad=pad, x_skew=skew)


def test_exact_data_long_rows_with_lds_hold(acc):
    """(2048,32768): a wavefront per row held to two workgroups per CU by its LDS request, vt_nsplit between 1 and its
    caps.  The data is drawn and the reference formed on the device: with exact products and sums every order of
    summation gives NumPy's bits, and the host would need seconds for its 512 MiB temporaries."""
    m, n, lamda = 2048, 32768, 0.37
    gen = torch.Generator(device="cuda").manual_seed(5)
    A = torch.randint(-8, 9, (m, n), generator=gen, device="cuda").to(torch.float64)
    x = torch.randint(-256, 257, (n,), generator=gen, device="cuda").to(torch.float64) / 64.0
    y = torch.randint(0, 2, (m,), generator=gen, device="cuda").to(torch.float64) * 2 - 1
    z = A @ x
    marg = y * z
    t = torch.clamp(1 - marg, min=0)
    r = torch.where(marg < 1, y, torch.zeros_like(y))
    F = float(t.sum()) / m + lamda / 2 * float(x @ x)
    g = (lamda * x - (r @ A) / m).cpu().numpy()
    f = acc.SVM_fun(lamda, A, y)
    v, gd = f.func_grad(x, 2)
    assert same_bits(v, F) and same_bits(gd.cpu().numpy(), g) and same_bits(f.margins(), z.cpu().numpy())
    assert same_bits(f.func_grad(x, 0), F)


def planted(m, n, seed):
    """rows 0..2 with y*z = 1, 1 - 1/64 and 1 + 1/64 exactly (x_0 = 1, x_1 = 1/64)"""
    A, x, y = exact_data(m, n, seed)
    x[0], x[1] = 1.0, 1.0 / 64
    for row, second, lab in ((0, 0.0, 1.0), (1, -1.0, 1.0), (2, 1.0, 1.0), (3, 0.0, -1.0)):
        if row < m:
            A[row] = 0.0
            A[row, 0] = lab
            A[row, 1] = second * lab
            y[row] = lab
    return A, x, y


@pytest.mark.parametrize("m,n", [(7, 129), (33, 4096)])
def test_planted_margins_pin_the_strict_less_and_the_max(acc, m, n):
    A, x, y = planted(m, n, 3)
    f = check_exact(acc, A, x, y, 0.5)
    xd = torch.from_numpy(x).cuda()
    f.func_grad(xd, 0)
    marg = y * f.margins()
    assert marg[0] == 1.0 and marg[1] == 1 - 1.0 / 64 and marg[2] == 1 + 1.0 / 64 and marg[3] == 1.0
    # a row at exactly 1 contributes nothing to the loss or the subgradient, the one below 1 contributes 1/64 and y*A
    A2, y2 = A[:4], y[:4]
    f2 = acc.SVM_fun(0.0, A2, y2)
    assert f2.hinge_loss(x) == (1.0 / 64) / 4
    sub = f2.subgradient_loss(x)
    want = np.zeros(n)
    want[0], want[1] = 1.0 / 4, -1.0 / 4
    assert same_bits(sub, want)


@pytest.mark.parametrize("m,n", [(5, 65), (33, 4096), (2050, 130)])
def test_nan_and_general_labels(acc, m, n):
    # y not +-1
    A, x, y = exact_data(m, n, 11, ymode="general")
    check_exact(acc, A, x, y, 0.37)
    # a NaN in one entry of A: the row's margin is NaN (kept by the max, "not < 1" for r), and 0*NaN reaches column j
    A, x, y = exact_data(m, n, 12)
    i, j = m // 2, n // 3
    A[i, j] = np.nan
    f = check_exact(acc, A, x, y, 0.37)
    v, g = f.func_grad(x, 2)
    assert np.isnan(v) and np.isnan(g[j]) and np.isnan(g).sum() == 1 and np.isnan(f.margins()).sum() == 1
    # a NaN in x: every margin is NaN, the subgradient is 0 and g = lamda*x
    A, x, y = exact_data(m, n, 13)
    x[n // 2] = np.nan
    f = check_exact(acc, A, x, y, 0.37)
    g = f.func_grad(x, 1)
    assert np.isnan(f(x)) and np.isnan(g).sum() == 1 and same_bits(np.delete(g, n // 2), 0.37 * np.delete(x, n // 2))
    assert same_bits(f.subgradient_loss(x), np.zeros(n))


def test_lamda_is_read_at_every_call_and_calls_repeat(acc):
    A, x, y = exact_data(33, 4096, 21)
    f = acc.SVM_fun(0.5, A, y)
    assert f.lamda == 0.5 and f.A is A and f.y is y
    a = f.func_grad(x, 2)
    f.lamda = 2.0
    b = f.func_grad(x, 2)
    assert same_bits(b[0], numpy_all(2.0, A, x, y)[0]) and same_bits(b[1], numpy_all(2.0, A, x, y)[2])
    assert not same_bits(a[1], b[1])
    # general data: two calls on the same input are bit-identical
    rng = np.random.RandomState(2)
    for m, n in [(96, 40), (33, 4100), (2050, 131)]:
        A, x = rng.randn(m, n), rng.randn(n) * 0.1
        y = rng.choice([-1.0, 1.0], size=m)
        f = acc.SVM_fun(0.3, A, y)
        v1, g1 = f.func_grad(x, 2)
        z1 = f.margins()
        v2, g2 = f.func_grad(x, 2)
        assert same_bits(v1, v2) and same_bits(g1, g2) and same_bits(z1, f.margins())
        assert same_bits(f.func_grad(x, 1), g1) and same_bits(f.func_grad(x, 0), v1)
    with pytest.raises(AssertionError):
        f.func_grad(np.zeros(5), 2)


def test_xx_has_the_bits_of_vec_dot(acc):
    """lamda/2*<x,x> is formed from the sum accbpg_vec_dot(x, x) returns: with A = 0 and y = 1 the hinge is exactly 1"""
    from accbpg_and_fw_amd.functions import vec_dot
    for n in (1, 255, 1025, 4097, 300001):
        x = T.draw(n, 3)
        f = acc.SVM_fun(2.0, np.zeros((2, n)), np.ones(2))
        xd = torch.from_numpy(x).cuda()
        assert f(xd) == 1.0 + 2.0 / 2 * vec_dot(xd, xd)
        assert vec_dot(xd, xd) == T.tree_sum(x * x, T.CAP_VEC)


def instance(tag, gold):
    if tag == "gauss":
        A, y = SN.gaussian_instance()
        np.testing.assert_allclose([A.sum(), np.abs(A).max(), (A ** 2).sum()], gold["gauss_A_checksum"], rtol=1e-14)
        return A, y
    return SN.digits_instance()


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("tag", ["gauss", "digits"])
def test_general_data_golden_points(acc, gold, tag, li):
    A, y = instance(tag, gold)
    m, n = A.shape
    key = "pc_%s_l%d" % (tag, li)
    lamda, pts = float(gold[key + "_lamda"]), gold[key + "_x"]
    f = acc.SVM_fun(lamda, A, y)
    absA = np.abs(A)
    for i, x in enumerate(pts):
        v, g = f.func_grad(x, 2)
        z = f.margins()
        assert np.min(np.abs(y * z - 1)) >= 1e-6 / 2
        ind = y * z < 1
        assert np.array_equal(ind, gold[key + "_ind"][i])
        hinge_ref = float(gold[key + "_hinge"][i])
        fb = gamma(n) * np.mean(absA.dot(np.abs(x))) + gamma(m) * hinge_ref + gamma(n) * (lamda / 2) * np.dot(x, x)
        df = abs(v - float(gold[key + "_fg_f"][i]))
        r = np.where(ind, y, 0).astype(np.float64)
        s_over_m = np.abs(gold[key + "_sub"][i])
        gb = gamma(m) * absA.T.dot(np.abs(r)) / m + 3 * U * (np.abs(lamda * x) + s_over_m)
        dg = np.abs(g - gold[key + "_fg_g"][i])
        print("%s point %d: |df| %.2e (bound %.2e)  max |dg|/bound %.3f" % (key, i, df, fb, np.max(dg / gb)))
        assert df <= fb
        assert np.all(dg <= gb)
        assert abs(f.hinge_loss(x) - hinge_ref) <= gamma(n) * np.mean(absA.dot(np.abs(x))) + gamma(m) * hinge_ref
        assert np.all(np.abs(f.subgradient_loss(x) - gold[key + "_sub"][i])
                      <= gamma(m) * absA.T.dot(np.abs(r)) / m + U * s_over_m)
        assert same_bits(f.func_grad(x, 1), g) and same_bits(f.func_grad(x, 0), v)


# ------------------------------------------------------------------------------------------------------- PolyDiv
def close(a, b, rel=1e-13):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    err = float(np.max(np.abs(a - b)) / np.max(np.abs(b)))
    assert err <= rel, err


@pytest.mark.parametrize("li", [0, 1])
@pytest.mark.parametrize("tag", ["gauss", "digits"])
def test_polydiv_values_against_restatement_and_goldens(acc, gold, tag, li):
    A, y = instance(tag, gold)
    key = "pc_%s_l%d" % (tag, li)
    lamda, radius, pts = float(gold[key + "_lamda"]), float(gold[key + "_radius"]), gold[key + "_x"]
    h, hr = acc.PolyDiv(A, lamda=lamda, radius=radius), SN.PolyDiv(A, lamda=lamda, radius=radius)
    assert h.DS_mean == hr.DS_mean and h.DS_mean_quad == hr.DS_mean_quad and h.lamda == lamda and h.radius == radius
    assert h.extra_Psi(pts[0]) == 0
    rng = np.random.RandomState(8)
    for i, x in enumerate(pts):
        w = pts[(i + 1) % 3]
        for ref_h, ref_g, ref_d in ((hr.h(x), hr.gradient(x), hr.divergence(x, w)),
                                    (gold[key + "_h"][i], gold[key + "_hgrad"][i], gold[key + "_hdiv"][i])):
            np.testing.assert_allclose(h.h(x), ref_h, rtol=1e-13)
            np.testing.assert_allclose(h(x), ref_h, rtol=1e-13)
            close(h.gradient(x), ref_g)
            np.testing.assert_allclose(h.divergence(x, w), ref_d, rtol=1e-13)
        g = rng.randn(x.size)
        xd, wd, gd = (torch.from_numpy(v).cuda() for v in (x, w, g))
        lin, dxy, dzz = h.ls_terms(gd, xd, wd, wd, xd)
        np.testing.assert_allclose(lin, np.dot(g, x - w), rtol=1e-12)
        np.testing.assert_allclose(dxy, hr.divergence(x, w), rtol=1e-13)
        np.testing.assert_allclose(dzz, hr.divergence(w, x), rtol=1e-13)
        from accbpg_and_fw_amd.algorithms import _divergences
        assert _divergences(h, gd, xd, wd, wd, xd) == (lin, dxy, dzz)
        for L in (0.05, 40.0):
            close(h.prox_map(g, L), hr.prox_map(g, L))
            close(h.div_prox_map(x, g, L), hr.div_prox_map(x, g, L))
    assert np.all(h.prox_map(np.zeros(5), 1.0) == 0)
    assert np.isnan(h.prox_map(np.r_[np.nan, np.ones(4)], 1.0)).all()
    assert np.isnan(h.div_prox_map(np.ones(5), np.r_[np.nan, np.ones(4)], 1.0)).all()


@pytest.mark.parametrize("n", T.edge_sizes(T.CAP_WIDE))
def test_polydiv_div_prox_map_at_the_tree_edges(acc, n):
    DS, _ = SN.gaussian_instance()
    lamda, radius = 0.5, 2.0
    h, hr = acc.PolyDiv(DS, lamda=lamda, radius=radius), SN.PolyDiv(DS, lamda=lamda, radius=radius)
    y = T.draw(n, 1) * (0.5 * radius / np.sqrt(n))
    g = T.draw(n, 2)
    for L in (1e-3, 2.0):                              # t^ beyond the radius / inside the ball
        x = h.div_prox_map(torch.from_numpy(y).cuda(), torch.from_numpy(g).cuda(), L).cpu().numpy()
        close(x, hr.div_prox_map(y, g, L))
        assert np.linalg.norm(x) <= radius * (1 + 1e-12)
    assert abs(np.linalg.norm(h.div_prox_map(y, g, 1e-3)) - radius) <= 1e-12 * radius


# ------------------------------------------------------------------------------------------------------ whole runs
def printed(text, col=2):
    rows = [ln.split() for ln in text.splitlines() if ln[:6].strip().isdigit()]
    return np.array([float(r[col]) for r in rows])


RUN_NAMES = list(SN.run_table(SN.SOLVERS, SN.lmo_l2_ball))


@pytest.mark.parametrize("name", RUN_NAMES)
@pytest.mark.parametrize("tag", ["gauss", "digits"])
def test_whole_runs_against_goldens(acc, gold, tag, name):
    A, y = instance(tag, gold)
    key = "run_" + tag
    lamda, L, radius, x0 = float(gold[key + "_lamda"]), float(gold[key + "_L"]), float(gold[key + "_radius"]), \
        gold[key + "_x0"]
    f = acc.SVM_fun(lamda, A, y)
    ph, sh = acc.PolyDiv(A, lamda=lamda, radius=radius), acc.SquaredL2Norm()
    key = "run_%s_%s" % (tag, name)
    buf = io.StringIO()
    np.random.seed(SN.RUN_SEED + RUN_NAMES.index(name))
    with contextlib.redirect_stdout(buf):
        x, F, G = SN.run_table(acc, acc.lmo_l2_ball)[name](f, ph, sh, L, np.copy(x0), radius)
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


DRIVER_NAMES = list(SN.driver_table(SN.SOLVERS, SN.lmo_l2_ball))


@pytest.mark.parametrize("name", DRIVER_NAMES)
def test_driver_calls_with_poly_h_against_restatement(acc, name):
    """The solver calls of the two ex_SVM drivers on the digits set with poly_h (40 iterations): the device run against
    the restatement's run in NumPy, which solves the same prox problems in closed form.  The Ls sequences are products
    of the line-search ratio and must agree to 1e-12; ABPG's G is a quotient of two divergences, each a difference of
    terms of the size of h, and is held to 1e-6."""
    X, Y = SN.digits_instance()
    lamda = 0.001 if name in ("aibm", "fgm") else 0.01            # aibm/ex_SVM.py:15, frank_wolfe_wtih_rs/ex_SVM.py:22
    np.random.seed(3)
    radius, _, _, L, x0 = SN.ball_numbers(X, Y, lamda)
    out = []
    for mod, lmo, fcls, hcls in ((acc, acc.lmo_l2_ball, acc.SVM_fun, acc.PolyDiv),
                                 (SN.SOLVERS, SN.lmo_l2_ball, SN.SVM_fun, SN.PolyDiv)):
        f, ph = fcls(lamda, X, Y), hcls(X, lamda=lamda, radius=radius)
        np.random.seed(77)
        with contextlib.redirect_stdout(io.StringIO()):
            out.append(SN.driver_table(mod, lmo)[name](f, ph, L, np.copy(x0), radius))
    (x, F, G), (xr, Fr, Gr) = out
    assert len(F) == len(Fr)
    dF = np.abs(F - Fr) / (1 + np.abs(Fr))
    print("driver %s: len %d  max dF %.2e  max dG %.2e" % (name, len(F), dF.max(), np.max(np.abs(G - Gr))))
    np.testing.assert_allclose(G, Gr, rtol=1e-6 if name == "abpg" else 1e-12)
    assert np.all(dF <= 1e-9)
    if name in ("fw", "bpgls", "abpg"):                             # iterates built from x0 and points of the ball
        assert np.linalg.norm(x) <= radius * (1 + 1e-12)


def test_factory_on_generated_data(acc):
    np.random.seed(5)
    f, (ph, sh), L, x0, radius = acc.svm_digits_ds_divs_ball(lamda=0.5)
    assert f.A.shape == (700, 2000) and f.y.shape == (700,) and x0.shape == (2000,)
    X = f.A
    assert radius == min(2000 ** -1 * 0.5 ** -1 * np.sum(np.linalg.norm(X[:, :-1], axis=1)), (2 / 0.5) ** 0.5)
    assert ph.radius == radius and ph.lamda == 0.5 and isinstance(sh, acc.SquaredL2Norm)
    assert L == (ph.DS_mean + min((2 * 0.5) ** 0.5, ph.DS_mean_quad)) * 0.08
    assert np.linalg.norm(x0) <= radius
    fr = SN.SVM_fun(0.5, X, f.y)
    v, g = f.func_grad(x0, 2)
    vr, gr = fr.func_grad(x0, 2)
    assert abs(v - vr) <= 1e-11 * abs(vr)
    if np.min(np.abs(f.y * fr.margins(x0) - 1)) > 1e-6:
        assert np.max(np.abs(g - gr)) <= 1e-11 * np.max(np.abs(gr))


def test_factory_on_the_digits_set(acc, gold):
    """real_ds=True loads the digits through scikit-learn (imported in that branch only): the reference's L, radius
    and x0 under its seed, and the data of the fixture"""
    pytest.importorskip("sklearn")
    pytest.importorskip("pandas")
    np.random.seed(3)
    f, (ph, sh), L, x0, radius = acc.svm_digits_ds_divs_ball(lamda=0.01, real_ds=True)
    X, Y = SN.digits_instance()
    assert np.array_equal(f.A, X) and np.array_equal(f.y, Y) and f.lamda == 0.01
    assert L == float(gold["fac_l0_L"]) and radius == float(gold["fac_l0_radius"])
    assert np.array_equal(x0, gold["fac_l0_x0"])
    assert ph.DS_mean == float(gold["fac_l0_DS_mean"]) and ph.DS_mean_quad == float(gold["fac_l0_DS_mean_quad"])
    assert abs(f(x0) - SN.SVM_fun(0.01, X, Y).F(x0)) <= 1e-12 * abs(f(x0))
