"""Host checks of tests/poisson_numpy.py, the helper of tests/test_gpu_poisson_forms.py: the generators are exact, the
measured allowance for log is the recorded one, the fp64 NumPy formulas of the reference stay below every bound at
every shape the GPU module runs (CU = 256), and the copied vt_nsplit has the values fw_kernels.hip gives by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poisson_numpy as PN  # noqa: E402

CU = 256
LD = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [s for s in PN.all_shapes(CU) if s[0] * s[1] <= 1 << 20]
BIG = [s for s in PN.all_shapes(CU) if s[0] * s[1] > 1 << 20]


def ratio(name, err, bound):
    err, bound = np.asarray(err, dtype=LD), np.asarray(bound, dtype=LD)
    assert np.all(bound > 0)
    r = float(np.max(err / bound))
    print("ratio to bound  %-32s %.4f" % (name, r))
    return r


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).nmant >= 63


def test_the_shape_lists():
    assert len(SMALL) + len(BIG) == len(PN.all_shapes(CU)) and len(BIG) == 4
    for s in [(1, 1), (5, 65), (7, 129), (33, 4096), (2050, 130), (416, 1540), (520, 130), (70001, 3)]:
        assert s in SMALL
    assert sorted(BIG) == [(2047, 4096), (2048, 4096), (2048, 32767), (2048, 32768)]


@pytest.mark.parametrize("m,n", SMALL)
def test_generators_are_exact(m, n):
    for gen, quot in ((PN.exact_poisson, lambda Ax, b, p: (b / Ax, p)), (PN.exact_kl, lambda Ax, b, p: (Ax / b, 1 / p))):
        A, x, p, b = gen(m, n, 100 * m + n)
        assert A.min() >= 1 and A.max() <= 8 and np.all(A == np.rint(A))
        assert x.min() >= 1 / 64 and x.max() <= 4 and np.all(x * 64 == np.rint(x * 64))
        Ax = A.dot(x)
        Axl = A.astype(LD).dot(x.astype(LD))
        assert np.array_equal(Ax.astype(LD), Axl)
        assert np.array_equal(b.astype(LD), Axl * p.astype(LD))
        q, want = quot(Ax, b, p)
        assert np.array_equal(q, want)
        assert set(np.unique(q)) <= set(PN.QUOTIENTS)
        # another order of summation gives the same A x
        assert np.array_equal(A[:, ::-1].dot(x[::-1]), Ax) and np.array_equal((A * x).sum(axis=1), Ax)
    # the Poisson gradient: the same bits in two orders and the np.longdouble result
    A, x, p, b = PN.exact_poisson(m, n, 100 * m + n)
    _, g, Ax = PN.poisson_fp64(A, x, b)
    r = 1 - b / Ax
    assert np.all(r * 4 == np.rint(r * 4))
    assert np.array_equal(g, r[::-1].dot(A[::-1])) and np.array_equal(g.astype(LD), PN.poisson_g_ref(A, Ax, b))
    # rows with p = 1 have t = 0, and with every p = 1 the reference's value and gradient are 0
    t = b * np.log(b / Ax) + Ax - b
    assert np.all(t[p == 1] == 0)
    for gen, fp64 in ((PN.exact_poisson, PN.poisson_fp64), (PN.exact_kl, PN.kl_fp64)):
        A, x, p, b = gen(m, n, 5, p_all_one=True)
        f, g, _ = fp64(A, x, b)
        assert f == 0 and not np.any(g)


def test_log_allowance_is_the_measured_one():
    worst = PN.measure_log()
    print("NumPy fp64 log against np.longdouble log: %.4f ulp" % worst)
    assert worst <= PN.LOG_MEASURED + 1e-3
    assert PN.LOG == int(np.ceil(PN.LOG_MEASURED)) + 1 == 2


def oracle_ratios(tag, A, x, pP, bP, pK, bK, S=None):
    m, n = A.shape
    out = {}
    f, g, Ax = PN.poisson_fp64(A, x, bP)
    fr, fb = PN.f_ref_and_bound(PN.poisson_terms, Ax, bP)
    out["poisson f"] = ratio("poisson f %s" % tag, abs(LD(f) - fr), fb)
    f, g, Ax = PN.kl_fp64(A, x, bK)
    fr, fb = PN.f_ref_and_bound(PN.kl_terms, Ax, bK)
    out["kl f"] = ratio("kl f %s" % tag, abs(LD(f) - fr), fb)
    gr, gb = PN.kl_g_ref_and_bound_grouped(PN.group_sums(A, pK), m)
    if np.any(pK != 1):
        out["kl g"] = ratio("kl g %s" % tag, np.abs(g.astype(LD) - gr), gb)
    if m * n <= 1 << 20:
        gd, gbd = PN.kl_g_ref_and_bound(A, Ax, bK)           # the grouped reference is the direct one
        sum_abs = gb / LD(PN.LOG * 2 * PN.U + PN.U + PN.gamma(m + 64))
        assert np.all(np.abs(gd - gr) <= (m + 8) * 2.0 ** -63 * sum_abs)
        assert np.all(np.abs(gbd - gb) <= 1e-15 * gb)
    return out


@pytest.mark.parametrize("m,n", SMALL)
def test_fp64_oracle_is_below_every_bound(m, n):
    A, x, pP, bP = PN.exact_poisson(m, n, 100 * m + n)
    A2, x2, pK, bK = PN.exact_kl(m, n, 100 * m + n)
    assert np.array_equal(A, A2) and np.array_equal(x, x2)
    for name, r in oracle_ratios("(%d,%d)" % (m, n), A, x, pP, bP, pK, bK).items():
        assert r < 1.0, (name, r)


@pytest.mark.parametrize("m,n", BIG)
def test_fp64_oracle_is_below_every_bound_long_rows(m, n):
    """the device-drawn shapes, with host data of the same kind"""
    rng = np.random.RandomState(m + n)
    A = rng.randint(1, 9, size=(m, n), dtype=np.int8).astype(np.float64)
    x = rng.randint(1, 257, size=n) / 64.0
    pP, pK = rng.choice(PN.P_POISSON, size=m), rng.choice(PN.P_KL, size=m)
    Ax = A.dot(x)
    for name, r in oracle_ratios("(%d,%d)" % (m, n), A, x, pP, Ax * pP, pK, Ax * pK).items():
        assert r < 1.0, (name, r)


def test_nonfinite_cases_have_the_classes_the_formulas_imply():
    """what the GPU module compares against in its non-finite cases"""
    A, x, p, b = PN.exact_poisson(5, 65, 1)
    b0 = b.copy()
    b0[2] = 0.0
    f, g, _ = PN.poisson_fp64(A, x, b0)
    assert np.isnan(f) and np.all(np.isfinite(g))
    f, g, _ = PN.kl_fp64(A, x, b0)
    assert f == np.inf and np.all(g == np.inf)
    bn = b.copy()
    bn[2] = -bn[2]
    f, g, _ = PN.poisson_fp64(A, x, bn)
    assert np.isnan(f) and np.all(np.isfinite(g))
    f, g, _ = PN.kl_fp64(A, x, bn)
    assert np.isnan(f) and np.all(np.isnan(g))
    f, g, _ = PN.poisson_fp64(A, 0 * x, b)
    assert f == np.inf and np.all(g == -np.inf)
    f, g, _ = PN.kl_fp64(A, 0 * x, b)
    assert np.isnan(f) and np.all(g == -np.inf)
    assert list(PN.classes([1.0, np.inf, -np.inf, np.nan, -0.0])) == [0, 1, 2, 3, 0]


# m, n -> vt_nsplit at CU = 256, from vt_nsplit of fw_kernels.hip by hand:
#   colblocks = ceil(n/512), s = (204 + colblocks/2) / colblocks, then min(s, 64, m/8), at least 1
NSPLIT_BY_HAND = {
    (1, 1): 1, (3, 2): 1, (4, 64): 1, (5, 65): 1, (7, 129): 1,             # m/8 = 0 -> 1
    (5, 4097): 1,                                                           # 9 blocks: 23, m/8 = 0 -> 1
    (33, 4096): 4, (33, 4095): 4,                                           # 8 blocks: 26, m/8 = 4
    (416, 1540): 51,                                                        # 4 blocks: 206/4 = 51 < m/8 = 52
    (2047, 4096): 26, (2048, 4096): 26,                                     # 8 blocks: 208/8 = 26
    (2048, 32768): 3, (2048, 32767): 3,                                     # 64 blocks: 236/64 = 3
    (2050, 130): 64, (520, 130): 64,                                        # 1 block: 204 -> 64; m/8 = 256, 65
    (1023, 3): 64, (1024, 3): 64, (1025, 3): 64, (70001, 3): 64,
}


def test_vt_nsplit_is_the_one_of_fw_kernels():
    shapes = PN.all_shapes(CU)
    assert set(shapes) == set(NSPLIT_BY_HAND)
    for s in shapes:
        assert PN.vt_nsplit(s[0], s[1], CU) == NSPLIT_BY_HAND[s], s
    # (520,130): 64 splits of 9 rows, 57 full ones and one of 7, the last six empty
    assert PN.empty_splits(520, 64) == [58, 59, 60, 61, 62, 63] and 57 * 9 + 7 == 520
    # the other shapes with empty splits: (416,1540) 51 splits of 9 rows, 46*9 = 414 < 416 <= 47*9; (2050,130) 64 of
    # 33 rows, 62*33 = 2046 < 2050 <= 63*33; (1025,3) 64 of 17 rows, 60*17 = 1020 < 1025 <= 61*17
    empty = {s: PN.empty_splits(s[0], NSPLIT_BY_HAND[s]) for s in shapes}
    assert empty.pop((520, 130)) and empty.pop((416, 1540)) == [47, 48, 49, 50] and empty.pop((2050, 130)) == [63]
    assert empty.pop((1025, 3)) == [61, 62, 63]
    assert all(v == [] for v in empty.values()), empty
    # the constants and the formula the copy restates
    text = open(os.path.join(ROOT, "accbpg_and_fw_amd", "csrc", "fw_kernels.hip")).read()
    for line in ("constexpr int FB = 256;", "constexpr int VG_COLS = 2 * FB;", "constexpr int VG_MAXSPLIT = 64;",
                 "const int64_t colblocks = (n + VG_COLS - 1) / VG_COLS;",
                 "int64_t s = (4 * (int64_t)num_cu / 5 + colblocks / 2) / colblocks;",
                 "if (s > VG_MAXSPLIT) s = VG_MAXSPLIT;", "if (s > m / 8) s = m / 8;", "if (s < 1) s = 1;",
                 "const int64_t rows_per = (m + nsplit - 1) / nsplit;"):
        assert line in text, line
    assert PN.VG_COLS == 512 and PN.VG_MAXSPLIT == 64


def test_launch_forms_on_the_host():
    forms = {s: PN.ax_form(s[0], s[1], CU) for s in PN.all_shapes(CU)}
    assert forms[(33, 4096)] == forms[(5, 4097)] == forms[(2047, 4096)] == "wg"
    assert forms[(33, 4095)] == forms[(2048, 4096)] == forms[(2050, 130)] == forms[(2048, 32767)] == "wave"
    assert forms[(2048, 32768)] == "hold"
    assert PN.loads_16(65, 66, False, False) == (True, True) and PN.loads_16(65, 67, False, False) == (False, False)
    assert PN.loads_16(64, 64, True, False) == (False, False) and PN.loads_16(64, 64, False, True) == (True, False)
