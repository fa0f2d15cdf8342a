"""GPU tests of the two row passes under PoissonRegression and KLdivRegression (poisson_kernels.hip, and the split-row
pass of fw_kernels.hip on this handle's own upart) on exact data, at the smallest shapes that reach each launch form.

Exact data (tests/poisson_numpy.py): A integers in [1, 8], x multiples of 1/64 in [1/64, 4], b = (A x) * p with p from
a short list of quotients.  A x, b, b/Ax = p (KL: Ax/b = 1/p) and the Poisson gradient A^T (1 - p) are exact in float64
in any order, so fitted() of both objectives and the Poisson gradient must have NumPy's bits, and f = 0, g = 0 where
every p_i = 1.  The Poisson value, the KL value and the KL gradient pass through log and are held to the forward
bounds derived in the helper's docstring, against np.longdouble evaluations of the reference's formulas.

Form -> shapes (CU = compute units of the device, 256 on MI355X):

  pass 1, a wavefront per row; rows per workgroup ragged (m mod 4 != 0); n/2 < 64     (1,1) (3,2) (4,64) (5,65) (7,129)
  pass 1, a wavefront per row because m >= 8*CU                                       (8*CU + 2, 130)
  pass 1, a workgroup per row (m < 8*CU and n >= 4096)                                (33,4096) (5,4097)
  the threshold in n from below                                                       (33,4095)
  the threshold in m at n = 4096                                                      (8*CU - 1, 4096) (8*CU, 4096)
  a wavefront per row with the LDS hold (n >= 32768)                                  (8*CU, 32768)
  no hold, one column below                                                           (8*CU, 32767) at lda 32768
  pass 2, vt_nsplit = 1                                                               (1,1) (3,2) (4,64) (5,65) (7,129)
          between its caps                                                            (416,1540) (8*CU, 32768)
          the m/8 cap                                                                 (33,4096)
          the 64 cap                                                                  (8*CU + 2, 130)
          empty splits                                                                (520,130): 64 splits of 9 rows,
                                                                                      splits 58 to 63 own no row
  poisson_fsum_kernel, one trip / more                                                m = 1023, 1024 / 1025, 70001 (n = 3)
  16-byte loads with the one-column tail (even lda > n, odd n)                        (5,65) at lda 66, (7,129) at 132,
                                                                                      (5,4097) at 4098, (8*CU, 32767)
  scalar loads (odd lda > n)                                                          (5,65) at 67, (33,4096) at 4101
  scalar loads (A at 8 mod 16, even lda)                                              (4,64) (5,65) at 66, (33,4096) at 4098
  scalar loads of pass 1, 16-byte loads of pass 2 (x at 8 mod 16)                     (4,64) (7,129) at 132 (33,4096)
                                                                                      (8*CU + 2, 130)

The strided and skewed cases go through the C-ABI (the classes always pass lda = n); every gap column holds NaN and
must not be read.  Shapes of more than a few million entries are drawn on the device and their references formed
there in float64 from exact products and sums (A @ x, r @ A, and for KL the five group sums of rows of equal p, from
which the np.longdouble gradient follows on the host).

Measured: the largest ratio of an error to its bound on MI355X, per quantity (every ratio is printed; the fp64 NumPy
formulas reach 0.044, 0.043 and 0.031 on the host):
  Poisson f   0.0443 at (5,4097)
  KL f        0.0429 at (1,1)
  KL g        0.0291 at (5,65)
The device's log stays well inside its share of two ulps.

Sensitivity, shown once on scratch copies of poisson_kernels.hip (each mutation reads inside the buffers):
  the odd-n tail line of the 16-byte path deleted: fails test_exact_data_strides_and_alignment at (5,65) lda 66,
    (7,129) lda 132, (5,4097) lda 4098, test_exact_data_long_rows_and_both_thresholds at (8*CU, 32767) and
    test_x_alignment_is_read_at_every_call, while the earlier Poisson, KL and inexact tests stay green;
  the scalar loop started at sub + TPR: fails 60 of the 90 tests here;
  b[row ^ 1] in the wave-per-row epilogue: fails 62 of the 90."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poisson_numpy as PN  # noqa: E402

pytestmark = pytest.mark.gpu
LD = np.longdouble
KINDS = ("poisson", "kl")
SENTINEL = -1234.5
RATIOS = {}


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def cu(acc):
    return torch.cuda.get_device_properties(0).multi_processor_count


def same_bits(a, b):
    """equal as float64 values, a NaN equal to a NaN (the sign of a zero is not compared)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _ratio(name, err, bound):
    """the largest err/bound; where the bound is 0 the error must be 0"""
    err, bound = np.atleast_1d(np.asarray(err, dtype=LD)), np.atleast_1d(np.asarray(bound, dtype=LD))
    assert np.all(bound >= 0) and np.all(err[bound == 0] == 0)
    pos = bound > 0
    r = float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0
    q = name.split(":")[0]
    RATIOS[q] = max(RATIOS.get(q, 0.0), r)
    print("ratio to bound  %-44s %.4f   (largest %s so far %.4f)" % (name, r, q, RATIOS[q]))
    return r


def gen(kind):
    return PN.exact_poisson if kind == "poisson" else PN.exact_kl


def cls(acc, kind):
    return acc.PoissonRegression if kind == "poisson" else acc.KLdivRegression


class Ref:
    """what f, g and fitted() are compared with: host data"""
    def __init__(self, kind, A, x, b):
        self.kind, self.m = kind, A.shape[0]
        if kind == "poisson":
            self.f64, self.g64, self.Ax = PN.poisson_fp64(A, x, b)
            self.f, self.fb = PN.f_ref_and_bound(PN.poisson_terms, self.Ax, b)
        else:
            self.f64, self.g64, self.Ax = PN.kl_fp64(A, x, b)
            self.f, self.fb = PN.f_ref_and_bound(PN.kl_terms, self.Ax, b)
            self.g, self.gb = PN.kl_g_ref_and_bound(A, self.Ax, b)

    def check(self, tag, f=None, g=None, ax=None):
        if ax is not None:
            assert same_bits(ax, self.Ax), tag
        if f is not None:
            assert _ratio("%s f: %s" % (self.kind, tag), abs(LD(f) - self.f), self.fb) <= 1.0
        if g is not None and self.kind == "poisson":
            assert same_bits(g, self.g64), tag
        elif g is not None:
            assert g.shape == self.g.shape
            assert _ratio("kl g: %s" % tag, np.abs(g.astype(LD) - self.g), self.gb) <= 1.0


def carve(v, skew):
    """a device copy of v at 16 bytes, or at 8 mod 16"""
    n = v.numel() if isinstance(v, torch.Tensor) else v.size
    buf = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    off = ((1 if skew else 0) - buf.data_ptr() // 8) % 2
    out = buf[off:off + n]
    out.copy_(v if isinstance(v, torch.Tensor) else torch.from_numpy(v))
    assert out.data_ptr() % 16 == (8 if skew else 0)
    return out


def place(A, pad, skew):
    """A in a NaN-filled device buffer with lda = n + pad, its base at 16 bytes or at 8 mod 16 -> (view, lda)"""
    m, n = A.shape
    lda = n + pad
    buf = torch.full((m * lda + 2,), float("nan"), dtype=torch.float64, device="cuda")
    off = ((1 if skew else 0) - buf.data_ptr() // 8) % 2
    Ad = buf[off:off + m * lda].view(m, lda)[:, :n]
    Ad.copy_(torch.from_numpy(A))
    assert Ad.data_ptr() % 16 == (8 if skew else 0)
    return Ad, lda


class Handle:
    """one objective handle through the C-ABI"""
    def __init__(self, kind, Ad, lda, bd):
        from accbpg_and_fw_amd import _lib
        self.lib = _lib.load()
        self.pre = "accbpg_poisson_" if kind == "poisson" else "accbpg_kldiv_"
        self.m, self.n = Ad.shape
        self.keep = (Ad, bd)
        self.h = C.c_void_p()
        torch.cuda.synchronize()
        rc = getattr(self.lib, self.pre + "create")(C.c_void_p(Ad.data_ptr()), self.m, self.n, lda,
                                                    C.c_void_p(bd.data_ptr()), None, C.byref(self.h))
        assert rc == 0

    def set_stream(self, stream):
        assert getattr(self.lib, self.pre + "set_stream")(self.h, C.c_void_p(stream) if stream else None) == 0

    def call(self, xd, flag, f_in=SENTINEL):
        """-> (*f_host after the call, g as NumPy or None)"""
        fv = C.c_double(f_in)
        g = torch.full((self.n,), SENTINEL, dtype=torch.float64, device="cuda") if flag else None
        torch.cuda.synchronize()
        rc = getattr(self.lib, self.pre + "func_grad")(self.h, C.c_void_p(xd.data_ptr()), flag, C.byref(fv),
                                                       C.c_void_p(g.data_ptr()) if flag else None)
        assert rc == 0
        torch.cuda.synchronize()
        return fv.value, (g.cpu().numpy() if flag else None)

    def fitted(self):
        out = torch.full((self.m,), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        assert getattr(self.lib, self.pre + "get_ax")(self.h, C.c_void_p(out.data_ptr())) == 0
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def close(self):
        if self.h:
            assert getattr(self.lib, self.pre + "destroy")(self.h) == 0
            self.h = None


# ---------------------------------------------------------------------------------------- every launch form, lda = n
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", PN.HOST_SHAPES, ids=str)
def test_exact_data_every_launch_form(acc, cu, kind, shape):
    m, n = PN.rows(shape, cu)
    A, x, p, b = gen(kind)(m, n, 100 * m + n)
    ref = Ref(kind, A, x, b)
    f = cls(acc, kind)(A, b)
    tag = "(%d,%d)" % (m, n)
    v2, g2 = f.func_grad(x, 2)
    ref.check(tag, v2, g2, f.fitted())
    v0 = f.func_grad(x, 0)
    assert same_bits(v0, v2) and same_bits(f.fitted(), ref.Ax)
    g1 = f.func_grad(x, 1)
    assert same_bits(g1, g2) and same_bits(f.fitted(), ref.Ax)
    assert same_bits(f(x), v2) and same_bits(f.gradient(x), g2)
    # a device x in, a device gradient out
    vd, gd = f.func_grad(torch.from_numpy(x).cuda(), 2)
    assert isinstance(gd, torch.Tensor) and same_bits(vd, v2) and same_bits(gd.cpu().numpy(), g2)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", [(5, 65), (7, 129), (33, 4096), ((8, 2), 130), (520, 130), (1025, 3)], ids=str)
def test_every_row_at_p_one_gives_zero(acc, cu, kind, shape):
    """b = A x: every t_i and every r_i is exactly 0, whatever the tree and the split"""
    m, n = PN.rows(shape, cu)
    A, x, p, b = gen(kind)(m, n, 3 * m + n, p_all_one=True)
    f = cls(acc, kind)(A, b)
    v, g = f.func_grad(x, 2)
    assert v == 0.0 and g.shape == (n,) and not np.any(g)
    assert same_bits(f.fitted(), A.dot(x)) and f.func_grad(x, 0) == 0.0 and not np.any(f.func_grad(x, 1))


def test_launch_forms_are_all_reached(acc, cu):
    """the shape lists hit both sides of every selecting condition of launch_ax, poisson_ax_kernel, vt_nsplit and
    poisson_fsum_kernel on this device"""
    shapes = [PN.rows(s, cu) for s in PN.HOST_SHAPES] + [PN.rows(s, cu) for s in PN.DEVICE_SHAPES]
    forms = {s: PN.ax_form(s[0], s[1], cu) for s in shapes}
    wg = [s for s in shapes if forms[s] == "wg"]
    wave = [s for s in shapes if forms[s] != "wg"]
    # m < 8*CU && n >= 4096, each side of each comparison with the other one true
    assert (33, 4096) in wg and (5, 4097) in wg and (8 * cu - 1, 4096) in wg
    assert (33, 4095) in wave and (8 * cu, 4096) in wave
    assert any(m >= 8 * cu and n < 4096 for m, n in wave) and any(m < 8 * cu and n < 4096 for m, n in wave)
    # n >= 32768 on the wavefront-per-row launch
    assert forms[(8 * cu, 32768)] == "hold" and forms[(8 * cu, 32767)] == "wave"
    # four rows per workgroup: a ragged last workgroup and a full one; rows shorter and longer than one trip of 64 lanes
    assert any(m % 4 for m, n in wave) and any(m % 4 == 0 for m, n in wave)
    assert any(n // 2 < 64 for m, n in wave) and any(n // 2 > 64 for m, n in wave)
    assert any(n // 2 > 256 for m, n in wg)
    # the load widths of the two passes, and the one-column tail under 16-byte loads
    cases = []                                              # (m, n, lda, A at 8 mod 16, x at 8 mod 16)
    for c in PN.STRIDE_CASES:
        m, n = PN.rows(c, cu)
        cases.append((m, n, n + c[2], c[3], c[4]))
    for s in PN.DEVICE_SHAPES:
        cases.append(PN.rows(s, cu) + (s[2], False, False))
    width = {c: PN.loads_16(*c[1:]) for c in cases}
    assert set(width.values()) == {(True, True), (True, False), (False, False)}
    for form in ("wg", "wave"):                             # 16-byte loads with and without the tail, both kernels
        for odd in (0, 1):
            assert any(w == (True, True) and c[1] % 2 == odd and PN.ax_form(c[0], c[1], cu) == form
                       for c, w in width.items()), (form, odd)
    assert any(w == (False, False) and c[3] and c[2] % 2 == 0 for c, w in width.items())     # the A base alone
    assert any(w == (False, False) and not c[3] and c[2] % 2 for c, w in width.items())      # the lda alone
    assert any(w == (True, False) and PN.ax_form(c[0], c[1], cu) == "wg" for c, w in width.items())
    assert any(w == (True, False) and PN.ax_form(c[0], c[1], cu) == "wave" for c, w in width.items())
    # pass 2: the splits
    splits = {s: PN.vt_nsplit(s[0], s[1], cu) for s in shapes}
    assert any(v == 1 for v in splits.values())
    assert any(v == s[0] // 8 and 1 < v < 64 for s, v in splits.items()), splits            # the m/8 cap
    assert any(1 < v < min(64, s[0] // 8) for s, v in splits.items()), splits               # in between
    assert any(v == 64 and s[0] // 8 > 64 for s, v in splits.items()), splits               # the 64 cap
    assert splits[(520, 130)] == 64 and PN.empty_splits(520, 64) == [58, 59, 60, 61, 62, 63]
    assert any(PN.empty_splits(s[0], v) == [] and v > 1 for s, v in splits.items())
    # poisson_fsum_kernel: one trip of 1024 lanes, its edge, more trips
    ms = [m for m, n in shapes]
    assert 1023 in ms and 1024 in ms and 1025 in ms and max(ms) > 64 * 1024


# ------------------------------------------------------------------------------------ long rows, drawn on the device
class Big:
    """the device-drawn shapes: data, references and one handle per (objective, shape), built once per module"""
    def __init__(self, cu):
        self.cu, self.data, self.inst = cu, {}, {}

    def matrix(self, i):
        if i not in self.data:
            m, n = PN.rows(PN.DEVICE_SHAPES[i], self.cu)
            lda = PN.DEVICE_SHAPES[i][2]
            g = torch.Generator(device="cuda").manual_seed(11 + i)
            buf = torch.randint(1, 9, (m, lda), generator=g, device="cuda", dtype=torch.float64)
            if lda > n:
                buf[:, n:] = float("nan")
            x = torch.randint(1, 257, (n,), generator=g, device="cuda", dtype=torch.float64) / 64.0
            Ad = buf[:, :n]
            Ax = Ad @ x
            assert not torch.isnan(Ax).any()
            self.data[i] = (Ad, lda, x, Ax, g)
        return self.data[i]

    def get(self, kind, i):
        if (kind, i) not in self.inst:
            Ad, lda, x, Ax, g = self.matrix(i)
            m, n = Ad.shape
            pset = torch.tensor(PN.P_POISSON if kind == "poisson" else PN.P_KL, dtype=torch.float64, device="cuda")
            k = torch.randint(0, pset.numel(), (m,), generator=g, device="cuda")
            p = pset[k]
            b = Ax * p
            Axh, bh = Ax.cpu().numpy(), b.cpu().numpy()
            ref = Ref.__new__(Ref)
            ref.kind, ref.m, ref.Ax = kind, m, Axh
            if kind == "poisson":
                assert same_bits((b / Ax).cpu().numpy(), p.cpu().numpy())
                ref.f, ref.fb = PN.f_ref_and_bound(PN.poisson_terms, Axh, bh)
                ref.g64 = ((1 - b / Ax) @ Ad).cpu().numpy()
            else:
                assert same_bits((Ax / b).cpu().numpy(), (1 / p).cpu().numpy())
                ref.f, ref.fb = PN.f_ref_and_bound(PN.kl_terms, Axh, bh)
                onehot = (k[None, :] == torch.arange(pset.numel(), device="cuda")[:, None]).to(torch.float64)
                ref.g, ref.gb = PN.kl_g_ref_and_bound_grouped((onehot @ Ad).cpu().numpy(), m)
            self.inst[(kind, i)] = (Handle(kind, Ad, lda, b), x, ref)
        return self.inst[(kind, i)]

    def close(self):
        for h, _, _ in self.inst.values():
            h.close()
        self.inst.clear()
        self.data.clear()
        torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def big(acc, cu):
    b = Big(cu)
    yield b
    b.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("i", range(len(PN.DEVICE_SHAPES)), ids=[str(s) for s in PN.DEVICE_SHAPES])
def test_exact_data_long_rows_and_both_thresholds(acc, big, kind, i):
    """(8*CU - 1, 4096) a workgroup per row against (8*CU, 4096) a wavefront per row; (8*CU, 32768) with the LDS hold
    against (8*CU, 32767) at lda 32768 without it, odd n under 16-byte loads, the last column of every row NaN.  With
    exact products and sums every order of summation gives the same bits, so the device's own float64 products are the
    reference."""
    h, x, ref = big.get(kind, i)
    tag = "(%d,%d)" % (h.m, h.n)
    v2, g2 = h.call(x, 2)
    ref.check(tag, v2, g2, h.fitted())
    v0, _ = h.call(x, 0)
    v1, g1 = h.call(x, 1)
    assert same_bits(v0, v2) and same_bits(g1, g2) and v1 == SENTINEL
    xs = carve(x, True)                                       # scalar loads of pass 1, the same bits
    vs, gs = h.call(xs, 2)
    assert same_bits(vs, v2) and same_bits(gs, g2) and same_bits(h.fitted(), ref.Ax)


# ------------------------------------------------------------------------------------ strides and alignment, C-ABI
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", PN.STRIDE_CASES, ids=str)
def test_exact_data_strides_and_alignment(acc, cu, kind, case):
    """an even lda > n with an odd n (16-byte loads and the one-column tail), an odd lda > n (scalar loads), an A base
    at 8 mod 16 under an even lda (scalar loads), an x at 8 mod 16 against an aligned A of even lda (scalar loads of
    pass 1, 16-byte loads of pass 2); the gap columns and the words around A hold NaN and must not be read"""
    (m, n), pad, a_skew, x_skew = PN.rows(case, cu), case[2], case[3], case[4]
    A, x, p, b = gen(kind)(m, n, 7 * m + n + pad)
    ref = Ref(kind, A, x, b)
    Ad, lda = place(A, pad, a_skew)
    h = Handle(kind, Ad, lda, torch.from_numpy(b).cuda())
    try:
        v, g = h.call(carve(x, x_skew), 2)
        ref.check("(%d,%d) lda %d A%+d x%+d" % (m, n, lda, 8 * a_skew, 8 * x_skew), v, g, h.fitted())
    finally:
        h.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n,pad", [(7, 129, 3), (33, 4096, 0), (5, 4097, 1)])
def test_x_alignment_is_read_at_every_call(acc, kind, m, n, pad):
    """one handle, x on 16 bytes, at 8 mod 16, on 16 bytes again: the load width of pass 1 follows the pointer of each
    call and all three return the same bits"""
    A, x, p, b = gen(kind)(m, n, 17 * m + n)
    ref = Ref(kind, A, x, b)
    Ad, lda = place(A, pad, False)
    h = Handle(kind, Ad, lda, torch.from_numpy(b).cuda())
    try:
        out = []
        for skew in (False, True, False):
            v, g = h.call(carve(x, skew), 2)
            out.append((v, g, h.fitted()))
        ref.check("(%d,%d) lda %d x 0/8/0" % (m, n, lda), *out[0])
        for v, g, ax in out[1:]:
            assert same_bits(v, out[0][0]) and same_bits(g, out[0][1]) and same_bits(ax, out[0][2])
    finally:
        h.close()


# --------------------------------------------------------------------------------------------- flags, repeats, stream
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", PN.FLAG_SHAPES)
def test_flags_repeats_and_stream(acc, kind, m, n):
    A, x, p, b = gen(kind)(m, n, 31 * m + n)
    x_other = 2 * x
    ref = Ref(kind, A, x, b)
    Ad, lda = place(A, 0, False)
    xd, xo = carve(x, False), carve(x_other, False)
    h = Handle(kind, Ad, lda, torch.from_numpy(b).cuda())
    try:
        v2, g2 = h.call(xd, 2)
        ax = h.fitted()
        ref.check("(%d,%d) flags" % (m, n), v2, g2, ax)
        # flag 1: the gradient of flag 2, *f_host untouched
        v1, g1 = h.call(xd, 1)
        assert v1 == SENTINEL and same_bits(g1, g2) and same_bits(h.fitted(), ax)
        v1, _ = h.call(xd, 1, f_in=float("inf"))
        assert v1 == np.inf
        # flag 0: the value of flag 2
        v0, _ = h.call(xd, 0)
        assert same_bits(v0, v2) and same_bits(h.fitted(), ax)
        # another x, then the first one again
        vo, go = h.call(xo, 2)
        axo = h.fitted()
        assert vo != v2 and not same_bits(go, g2) and not same_bits(axo, ax)
        assert same_bits(axo, A.dot(x_other))                 # b/(2 A x) = p/2 is exact too: the Poisson bits
        if kind == "poisson":
            assert same_bits(go, PN.poisson_fp64(A, x_other, b)[1])
        vo1, go1 = h.call(xo, 2)
        assert same_bits(vo1, vo) and same_bits(go1, go)
        vr, gr = h.call(xd, 2)
        assert same_bits(vr, v2) and same_bits(gr, g2) and same_bits(h.fitted(), ax)
        # a stream of the caller's
        s = torch.cuda.Stream()
        h.set_stream(s.cuda_stream)
        vs, gs = h.call(xd, 2)
        assert same_bits(vs, v2) and same_bits(gs, g2) and same_bits(h.fitted(), ax)
        vs0, _ = h.call(xd, 0)
        _, gs1 = h.call(xd, 1)
        assert same_bits(vs0, v2) and same_bits(gs1, g2)
        h.set_stream(None)
        vn, gn = h.call(xd, 2)
        assert same_bits(vn, v2) and same_bits(gn, g2)
        # the classes pass the current stream at every call
        f = cls(acc, kind)(A, b)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            vc, gc = f.func_grad(xd, 2)
            vc0, gc1 = f.func_grad(xd, 0), f.func_grad(xd, 1)
            axc = f.fitted()
        s.synchronize()
        assert same_bits(vc, v2) and same_bits(gc.cpu().numpy(), g2) and same_bits(axc, ax)
        assert same_bits(vc0, v2) and same_bits(gc1.cpu().numpy(), g2)
        vd, gd = f.func_grad(xd, 2)
        assert same_bits(vd, v2) and same_bits(gd.cpu().numpy(), g2)
    finally:
        h.close()


# --------------------------------------------------------------------------------------------------- non-finite values
def nonfinite_cases(A, x, b):
    m, n = A.shape
    b0 = b.copy()
    b0[m // 2] = 0.0
    bn = b.copy()
    bn[m // 3] = -bn[m // 3]
    xn = x.copy()
    xn[n // 2] = np.nan
    return [("b_i = 0", x, b0), ("b_i < 0", x, bn), ("NaN in x", xn, b), ("x = 0", np.zeros(n), b)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("m,n", PN.NONFINITE_SHAPES)
def test_nonfinite_values_have_numpys_class(acc, kind, m, n):
    """A >= 1 everywhere, so 0*inf cannot arise in a product with A: f and every g_j must be finite, +inf, -inf or NaN
    as the NumPy formulas are, and within the bounds where finite (the Poisson gradient: NumPy's bits, r stays exact)"""
    A, x, p, b = gen(kind)(m, n, 41 * m + n)
    seen = set()
    for name, xc, bc in nonfinite_cases(A, x, b):
        with np.errstate(all="ignore"):
            ref = Ref(kind, A, xc, bc)
        f = cls(acc, kind)(A, bc)
        v, g = f.func_grad(xc, 2)
        tag = "(%d,%d) %s" % (m, n, name)
        fc, gc = int(PN.classes(ref.f64)[0]), PN.classes(ref.g64)
        print("%s %s: f %r (NumPy %r), classes of g %s" % (kind, tag, v, float(ref.f64), sorted(set(gc.tolist()))))
        assert int(PN.classes(v)[0]) == fc, tag
        assert np.array_equal(PN.classes(g), gc), tag
        assert same_bits(f.fitted(), ref.Ax), tag
        if fc == 0:
            assert _ratio("%s f: %s" % (kind, tag), abs(LD(v) - ref.f), ref.fb) <= 1.0
        fin = gc == 0
        if fin.any() and kind == "poisson":
            assert same_bits(g[fin], ref.g64[fin]), tag
        elif fin.any():
            assert _ratio("kl g: %s" % tag, np.abs(g[fin].astype(LD) - ref.g[fin]), ref.gb[fin]) <= 1.0
        assert same_bits(f.func_grad(xc, 0), v) and same_bits(f.func_grad(xc, 1), g)
        seen.add((fc, tuple(sorted(set(gc.tolist())))))
    want = {"poisson": {(3, (0,)), (3, (3,)), (1, (2,))}, "kl": {(1, (1,)), (3, (3,)), (3, (2,))}}[kind]
    assert seen == want, seen


def test_zz_report_measured_ratios():
    """the largest ratio per quantity over the module, for the docstring above"""
    for q in sorted(RATIOS):
        print("Measured: largest ratio to bound  %-10s %.4f" % (q, RATIOS[q]))
    assert all(r <= 1.0 for r in RATIOS.values())
