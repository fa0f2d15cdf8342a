"""Guard bands around the caller-owned buffers of the C-ABI (tests/guard_arena.py): every entry point that takes a device
output or a workspace is called with pointers carved out of one sentinel-filled arena -- a band in front of and behind
every buffer, the gap columns [cols, ld) of every matrix, the workspace exactly accbpg_vec_workspace_doubles(n) long --
and then (i) every double outside the buffers the header names as written has its bits unchanged, the inputs included,
(ii) an output that is written whole holds no sentinel any more, and (iii) the results equal those of the same call on
plain torch allocations:
  * 16-byte-aligned carves, and 8-mod-16 ("skewed") carves of the length-n kernels: bit for bit (one fixed tree,
    ordered by index);
  * skewed x of the D-optimal entries, which pick a kernel by alignment (launch_gram: `xal`): the tolerance of
    test_gpu_parity.py::test_gram_unaligned_x_through_c_abi -- every scalar within 1e-11 relative of its own value,
    every vector element by element at rtol = 1e-11 (atol = 0), and the m x m matrices, which that test does not have,
    within 1e-11 of their largest entry.
Shapes: the sizes at which the launch forms change (reduce_numpy.edge_sizes, prox_numpy.PRODUCTION, the second trip of
the elementwise passes) and the ragged / chain / split-K / fused shapes of the D-optimal tests."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402
import prox_numpy as PN  # noqa: E402
import reduce_numpy as T  # noqa: E402

pytestmark = pytest.mark.gpu

EW_SECOND_TRIP = 2048 * 256 + 1         # the first size at which the elementwise passes make a second trip
PROX_SIZES = sorted({n for _, n in PN.PRODUCTION} | {32769})


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from accbpg_and_fw_amd import _lib
    return _lib.load()


def err():
    from accbpg_and_fw_amd import _lib
    return _lib.last_error()


def P(v):
    return C.c_void_p(v.ptr) if v is not None else None


def f64(*vals):
    return np.array(vals, dtype=np.float64)


_DATA = {}


def data(n):
    """device vectors of length n, drawn once and never written: g x y z w of mixed sign, pg .. pw positive, sx / sz
    positive with sum 1"""
    if n not in _DATA:
        h = {}
        for k, name in enumerate("gxyzw"):
            v = T.draw(n, k)
            h[name] = v
            h["p" + name] = np.abs(v) + 0.05
        h["sx"] = h["px"] / h["px"].sum()
        h["sz"] = h["pz"] / h["pz"].sum()
        h["gnorm"] = float(np.linalg.norm(h["g"]))
        dev = {k: torch.from_numpy(v).cuda() for k, v in h.items() if isinstance(v, np.ndarray)}
        dev["gnorm"] = h["gnorm"]
        if len(_DATA) > 6:
            _DATA.pop(next(iter(_DATA)))
        _DATA[n] = dev
    return _DATA[n]


# ------------------------------------------------------------------------------------------------- the runner
_PLAIN = {}


def run_case(case, key, skew, tol=None):
    """case(A) carves from allocator A, calls A.snapshot(), makes its calls, calls A.check(...) and returns a list of
    (name, array).  Run on plain tensors (once per key) and on an arena; the results must agree bit for bit, except the
    results named in tol (where the docstring above allows a tolerance): tol[name] = ("each", r) holds every entry
    within r relative of the plain call's entry (scalars, vectors), ("norm", r) within r of the largest entry (m x m
    matrices)."""
    if key not in _PLAIN:
        _PLAIN.clear()                          # the cases of one key follow each other
        _PLAIN[key] = case(GA.Plain())
    want = _PLAIN[key]
    got = case(GA.Arena())
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if tol is None or name not in tol:
            same = a.view(np.int64) == b.view(np.int64) if a.dtype == np.float64 else a == b
            assert np.all(same), "%s: %d of %d entries differ from the plain call (first at %d)" % (
                name, int(np.sum(~same)), same.size, int(np.flatnonzero(~np.ravel(same))[0]))
            continue
        how, r = tol[name]
        fa, fb = a.view(np.float64), b.view(np.float64)
        assert np.all(np.isfinite(fa)) and np.all(np.isfinite(fb)), name
        dev = np.abs(fa - fb)
        bound = r * np.abs(fb) if how == "each" else r * float(np.max(np.abs(fb)))
        print("%s: max deviation %.3e, %d entries differ in bits" % (name, float(dev.max()), int(np.sum(fa != fb))))
        assert np.all(dev <= bound), (name, how, float(np.max(dev - bound)))


def ok(rc, what):
    assert rc == 0, "%s returned %d: %s" % (what, rc, err())


def sizes_with_skew(sizes):
    """every size at skew 0, the three smallest and the largest at skew 1 too (right behind: the plain call is shared)"""
    sizes = sorted(sizes)
    return [(n, sk) for n in sizes for sk in ((0, 1) if n in sizes[:3] + sizes[-1:] else (0,))]


def ws_of(lib, A, n, skew):
    return A.carve(lib.accbpg_vec_workspace_doubles(n), skew=skew, name="ws")


# ------------------------------------------------------------------------------------------------- the harness itself
def test_harness_reports_a_stray_double_with_its_offset():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    A = GA.Arena(40000)
    a = A.carve(100, data=np.arange(100.0), name="a")
    b = A.carve(7, skew=1, name="b")
    M = A.carve2d(5, 6, 9, data=np.ones((5, 6)), name="M")
    assert a.ptr % 16 == 0 and b.ptr % 16 == 8 and M.t.stride() == (9, 1)
    assert int((A.bits == GA.SENTINEL).sum()) == A.bits.numel() - 100 - 30
    A.snapshot()
    A.check(writable=[b])                                           # a clean arena passes
    assert A.damage() is None
    b.t[:] = 1.0
    A.check(writable=[b], whole=[b])
    with pytest.raises(GA.GuardError) as e:                         # ... and an output nobody named is damage
        A.check(writable=[])
    assert (e.value.name, e.value.side, e.value.offset) == ("b", "inside", 0)
    b.t[3] = float("nan")                                           # any other NaN is not the sentinel
    A.check(writable=[b], whole=[b])
    b.t.view(torch.int64)[3] = GA.SENTINEL
    with pytest.raises(GA.GuardError) as e:
        A.check(writable=[b], whole=[b])
    assert (e.value.name, e.value.side, e.value.offset) == ("b", "unwritten", 3)
    b.t[3] = 2.0

    def stray(index, value=0.0):
        old = A.bits[index].clone()
        A.buf[index] = value
        with pytest.raises(GA.GuardError) as e:
            A.check(writable=[b, M])
        A.bits[index] = old
        A.check(writable=[b, M])
        return e.value.name, e.value.side, e.value.offset

    assert stray(a.off + 100) == ("a", "behind", 100)               # just past a view
    assert stray(a.off - 1) == ("a", "front", -1)                   # just in front of one
    assert stray(b.off + 7) == ("b", "behind", 7)
    assert stray(b.off - 1) == ("b", "front", -1)
    assert stray(M.off + 2 * 9 + 6) == ("M", "gap", 2 * 9 + 6)      # the first gap column of row 2
    assert stray(M.off + 4 * 9 + 6) == ("M", "behind", 4 * 9 + 6)   # behind the last row's last column
    assert stray(a.off + 5) == ("a", "inside", 5)                   # an input was modified
    assert "row 2, column 6" in str(_raise(A, M.off + 2 * 9 + 6, [b, M]))
    # a matrix named writable covers its elements, never its gaps
    M.t[:] = 3.0
    A.check(writable=[b, M], whole=[M])
    assert int((A.bits == GA.SENTINEL).sum()) == A.bits.numel() - 100 - 7 - 30


def _raise(A, index, writable):
    old = A.bits[index].clone()
    A.buf[index] = 0.0
    try:
        A.check(writable=writable)
    except GA.GuardError as e:
        return e
    finally:
        A.bits[index] = old
    raise AssertionError("not reported")


# ------------------------------------------------------------------------------------------------- length-n entries
# Each entry: case(lib, A, n, skew) -> results.  `s` carves an input, `o` an output, both at the case's skew.
def _io(A, skew):
    def s(name, t):
        return A.carve(t.numel(), data=t, skew=skew, name=name)

    def o(name, count):
        return A.carve(count, skew=skew, name=name)
    return s, o


def burg_simplex_prox(with_y):
    def case(lib, A, n, skew):
        d = data(n)
        s, o = _io(A, skew)
        y = s("y", d["sx"]) if with_y else None
        g = s("g", d["g"])
        x = o("x_out", n)
        ws = ws_of(lib, A, n, skew)
        info = (C.c_int * 2)()
        A.snapshot()
        ok(lib.accbpg_burg_simplex_div_prox(P(y), P(g), 1.5, 1e-8, n, P(x), P(ws), info, None), "burg_simplex_div_prox")
        A.check(writable=[x, ws], whole=[x])
        return [("x_out", A.bits_of(x)), ("info", np.array(list(info), dtype=np.int64))]
    return case


def burg_prox_acc(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    xi, g = s("xi", d["px"]), s("g", d["g"])
    xo, x = o("xi_out", n), o("x_out", n)
    ws = ws_of(lib, A, n, skew)
    info = (C.c_int * 2)()
    A.snapshot()
    ok(lib.accbpg_burg_simplex_prox_acc(P(xi), 0.01, P(g), 1.5, 1e-8, n, P(xo), P(x), P(ws), info, None), "prox_acc")
    A.check(writable=[xo, x, ws], whole=[xo, x])
    return [("xi_out", A.bits_of(xo)), ("x_out", A.bits_of(x)), ("info", np.array(list(info), dtype=np.int64))]


def burg_family(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    g, pg, x, y, z, z1 = s("g", d["g"]), s("pg", d["pg"]), s("x", d["px"]), s("y", d["py"]), s("z", d["pz"]), s("z1", d["pw"])
    outs = [o("reg%d%s" % (k, "y" if wy else ""), n) for k in (0, 1, 2) for wy in (0, 1)]
    ws = ws_of(lib, A, n, skew)
    A.snapshot()
    res = []
    out = (C.c_double * 3)()
    ok(lib.accbpg_burg_divergence(P(x), P(y), n, out, P(ws), None), "burg_divergence")
    res.append(("divergence", f64(out[0])))
    ok(lib.accbpg_ls_terms(P(g), P(x), P(y), P(z), P(z1), n, out, P(ws), None), "ls_terms")
    res.append(("ls_terms", f64(*out)))
    ok(lib.accbpg_ls_terms(None, P(x), P(y), None, None, n, out, P(ws), None), "ls_terms")
    res.append(("ls_terms_xy", f64(*out)))
    A.check(writable=[ws])
    it = iter(outs)
    for kind in (0, 1, 2):
        for wy in (0, 1):
            v = next(it)
            ok(lib.accbpg_burg_reg_div_prox(kind, P(y) if wy else None, P(pg), 1.5, 0.25, n, P(v), None), "burg_reg_div_prox")
            res.append((v.name, A.bits_of(v)))
    A.check(writable=[ws] + outs, whole=outs)
    return res


def vec_family(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    g, x, y = s("g", d["g"]), s("x", d["x"]), s("y", d["y"])
    ax, dv, vx, cnt = o("axpby", n), o("div", n), o("vertex", n), o("count", 1)
    ws = ws_of(lib, A, n, skew)
    A.snapshot()
    out = (C.c_double * 2)()
    res = []
    ok(lib.accbpg_vec_axpby(0.3, P(x), 0.7, P(y), n, P(ax), None), "axpby")
    ok(lib.accbpg_vec_div_scalar(P(x), 3.0, n, P(dv), None), "div_scalar")
    ok(lib.accbpg_vec_vertex(n - 1, 0.5, 1e-15, n, P(vx), None), "vertex")
    ok(lib.accbpg_vec_count_bad(P(x), n, P(cnt), None), "count_bad")
    A.check(writable=[ax, dv, vx, cnt], whole=[ax, dv, vx, cnt])
    ok(lib.accbpg_vec_dot_diff(P(g), P(x), P(y), n, out, P(ws), None), "dot_diff")
    res.append(("dot_diff", f64(out[0])))
    ok(lib.accbpg_vec_dot(P(x), P(y), n, out, P(ws), None), "dot")
    res.append(("dot", f64(out[0])))
    ok(lib.accbpg_vec_min_sum(P(x), n, out, P(ws), None), "min_sum")
    res.append(("min_sum", f64(*out)))
    A.check(writable=[ax, dv, vx, cnt, ws])
    return res + [(v.name, A.bits_of(v)) for v in (ax, dv, vx, cnt)]


def argminmax(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    x = s("x", d["x"])
    ws = ws_of(lib, A, n, skew)
    idx, val = (C.c_int64 * 2)(), (C.c_double * 2)()
    A.snapshot()
    ok(lib.accbpg_vec_argminmax(P(x), n, idx, val, P(ws), None), "argminmax")
    A.check(writable=[ws])
    return [("idx", np.array(list(idx), dtype=np.int64)), ("val", f64(*val))]


def inexact_family(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    g, u, v, x, pu, pv, px = (s(k, d[k]) for k in ("g", "x", "y", "z", "px", "py", "pz"))
    w0, w1, wn, lo = o("w_burg", n), o("w_l2", n), o("w_only", n), o("lmo_pos", n)
    ws = ws_of(lib, A, n, skew)
    A.snapshot()
    out = (C.c_double * 3)()
    res = []
    ok(lib.accbpg_combine_ls_terms(0, 0.3, P(pu), 0.7, P(pv), 1.3, P(g), P(px), n, P(w0), out, P(ws), None), "combine 0")
    res.append(("combine_burg", f64(out[0], out[1])))
    ok(lib.accbpg_combine_ls_terms(1, 0.3, P(u), 0.7, P(v), 1.3, P(g), P(x), n, P(w1), out, P(ws), None), "combine 1")
    res.append(("combine_l2", f64(out[0], out[1])))
    ok(lib.accbpg_combine_ls_terms(1, 0.3, P(u), 0.7, P(v), 1.0, None, None, n, P(wn), None, None, None), "combine x=NULL")
    ok(lib.accbpg_lmo_l2_ball_pos(P(g), P(px), 1.0, 1e-6, n, P(lo), out, P(ws), None), "lmo_l2_ball_pos")
    res.append(("lmo_pos_info", f64(*out)))
    outs = [w0, w1, wn, lo]
    A.check(writable=outs + [ws], whole=outs)
    return res + [(t.name, A.bits_of(t)) for t in outs]


def shannon_family(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    g, x, y, z, z1 = s("g", d["g"]), s("x", d["px"]), s("y", d["py"]), s("z", d["pz"]), s("z1", d["pw"])
    outs = [o("prox%d%s" % (k, "y" if wy else ""), n) for k in (0, 1, 2) for wy in (0, 1)]
    ws = ws_of(lib, A, n, skew)
    A.snapshot()
    res = []
    it = iter(outs)
    for kind in (0, 1, 2):
        for wy in (0, 1):
            t = next(it)
            ok(lib.accbpg_shannon_div_prox(kind, P(y) if wy else None, P(g), 1.5, 0.25, n, P(t), P(ws), None),
               "shannon_div_prox")
    A.check(writable=outs + [ws], whole=outs)
    out = (C.c_double * 3)()
    ok(lib.accbpg_shannon_ls_terms(P(g), P(x), P(y), P(z), P(z1), n, 1e-20, out, P(ws), None), "shannon_ls_terms")
    res.append(("ls_terms", f64(*out)))
    ok(lib.accbpg_shannon_ls_terms(None, P(x), P(y), None, None, n, 1e-20, out, P(ws), None), "shannon_ls_terms")
    res.append(("ls_terms_xy", f64(*out)))
    ok(lib.accbpg_shannon_divergence(P(x), P(y), n, 1e-20, out, P(ws), None), "shannon_divergence")
    res.append(("divergence", f64(out[0])))
    A.check(writable=outs + [ws])
    return res + [(t.name, A.bits_of(t)) for t in outs]


def quartic_family(lib, A, n, skew):
    d = data(n)
    s, o = _io(A, skew)
    g, x, y, z, z1 = s("g", d["g"]), s("x", d["x"]), s("y", d["y"]), s("z", d["z"]), s("z1", d["w"])
    outs = [o(k, n) for k in ("stage0", "stage1", "l2_val", "l2_vec", "linf_val", "linf_vec")]
    ws = ws_of(lib, A, n, skew)
    A.snapshot()
    res = []
    out = (C.c_double * 7)()
    ok(lib.accbpg_quartic_prox_stage(P(y), P(g), 1.7, 0.37, 0, float("inf"), n, P(outs[0]), out, P(ws), None), "stage 0")
    res.append(("ssq0", f64(out[0])))
    ok(lib.accbpg_quartic_prox_stage(P(y), P(g), 1.7, 0.37, 1, 0.9, n, P(outs[1]), out, P(ws), None), "stage 1")
    res.append(("ssq1", f64(out[0])))
    ok(lib.accbpg_quartic_ls_terms(P(g), P(x), P(y), P(z), P(z1), n, out, P(ws), None), "quartic_ls_terms")
    res.append(("ls_terms", f64(*out)))
    gn = d["gnorm"]
    ok(lib.accbpg_lmo_l2_ball(P(g), 0, None, 0.25, 1.0, gn, n, P(outs[2]), out, P(ws), None), "lmo_l2_ball value centre")
    res.append(("dist_val", f64(out[0])))
    ok(lib.accbpg_lmo_l2_ball(P(g), 1, P(x), 0.0, 1.0, gn, n, P(outs[3]), out, P(ws), None), "lmo_l2_ball vector centre")
    res.append(("dist_vec", f64(out[0])))
    ok(lib.accbpg_lmo_linf_ball(P(g), 0, None, 0.25, 1.0, n, P(outs[4]), None), "lmo_linf_ball value centre")
    ok(lib.accbpg_lmo_linf_ball(P(g), 1, P(x), 0.0, 1.0, n, P(outs[5]), None), "lmo_linf_ball vector centre")
    A.check(writable=outs + [ws], whole=outs)
    return res + [(t.name, A.bits_of(t)) for t in outs]


VEC_SIZES = T.edge_sizes(T.CAP_VEC) + [EW_SECOND_TRIP]
WIDE_SIZES = T.edge_sizes(T.CAP_WIDE) + [EW_SECOND_TRIP]
FAMILIES = [("burg", burg_family, VEC_SIZES), ("vec", vec_family, VEC_SIZES), ("inexact", inexact_family, VEC_SIZES),
            ("argminmax", argminmax, T.edge_sizes(T.CAP_ARG)), ("shannon", shannon_family, WIDE_SIZES),
            ("quartic", quartic_family, WIDE_SIZES), ("prox_y", burg_simplex_prox(True), PROX_SIZES),
            ("prox", burg_simplex_prox(False), PROX_SIZES), ("prox_acc", burg_prox_acc, PROX_SIZES)]


@pytest.mark.parametrize("name,n,skew", [(name, n, sk) for name, _, sizes in FAMILIES for n, sk in sizes_with_skew(sizes)])
def test_length_n_entries(lib, name, n, skew):
    fn = next(f for k, f, _ in FAMILIES if k == name)
    run_case(lambda A: fn(lib, A, n, skew), (name, n), skew)


# ------------------------------------------------------------------------------------------------- packed triangle
@pytest.mark.parametrize("m", [1, 13, 64, 65, 257, 333])
@pytest.mark.parametrize("skew", [0, 1])
def test_tri_pack_and_unpack(lib, m, skew):
    rng = np.random.RandomState(m)
    G0, U0 = rng.randn(m, m), rng.randn(m, m)

    def case(A):
        G = A.carve2d(m, m, m, data=G0, skew=skew, name="G")
        packed = A.carve(m * (m + 1) // 2, skew=skew, name="packed")            # exactly the message
        U = A.carve2d(m, m, m, data=U0, skew=skew, name="unpacked")
        A.snapshot()
        ok(lib.accbpg_tri_pack(P(G), m, P(packed), None), "tri_pack")
        A.check(writable=[packed], whole=[packed])
        ok(lib.accbpg_tri_unpack(P(packed), m, P(U), None), "tri_unpack")
        A.check(writable=[packed, U])
        return [("packed", A.bits_of(packed)), ("unpacked", A.bits_of(U))]

    run_case(case, ("tri", m, skew), skew)
    got = _PLAIN[("tri", m, skew)]
    np.testing.assert_array_equal(got[0][1].view(np.float64), G0[np.tril_indices(m)])
    # unpack writes the lower triangle and leaves the strict upper one as it was (accbpg_hip.h: "only the lower
    # triangle ... is significant")
    np.testing.assert_array_equal(got[1][1].view(np.float64).reshape(m, m), np.tril(G0) + np.triu(U0, 1))


# ------------------------------------------------------------------------------------------------- the MFMA engine
@pytest.mark.parametrize("config", [0, 1])
@pytest.mark.parametrize("kmajor", [0, 1])
@pytest.mark.parametrize("shape", [(64, 64, 64), (256, 128, 48), (300, 200, 77), (129, 65, 33), (512, 384, 1000), (17, 5, 3)])
def test_gemm_engine_inside_ldc(lib, config, kmajor, shape):
    """the shapes of test_mfma_gemm_matches_numpy with ldc > N (and lda, ldb wider than their rows): the masked tile
    stores may not reach the gap columns of C, and rows M .. of the last tile are band.  C is read and written
    (accbpg_hip.h: C <- alpha * A * op(B) + beta * C)."""
    M, N, K = shape
    rng = np.random.RandomState(M * 7 + N * 3 + K)
    A0 = rng.randn(M, K)
    B0 = rng.randn(K, N) if kmajor else rng.randn(N, K)
    C0 = rng.randn(M, N)
    lda, ldb, ldc = K + 2, B0.shape[1] + 4, N + 6

    def case(Al):
        Av = Al.carve2d(M, K, lda, data=A0, name="A")
        Bv = Al.carve2d(B0.shape[0], B0.shape[1], ldb, data=B0, name="B")
        Cv = Al.carve2d(M, N, ldc, data=C0, name="C")
        Al.snapshot()
        ok(lib.accbpg_test_gemm(P(Av), lda, P(Bv), ldb, P(Cv), ldc, M, N, K, kmajor, -1.25, 0.5, config, None), "test_gemm")
        Al.check(writable=[Cv], whole=[Cv])
        return [("C", Al.bits_of(Cv))]

    run_case(case, ("gemm", config, kmajor, shape), 0)
    got = _PLAIN[("gemm", config, kmajor, shape)][0][1].view(np.float64).reshape(M, N)
    ref = -1.25 * (A0 @ (B0 if kmajor else B0.T)) + 0.5 * C0
    scale = np.abs(A0) @ np.abs(B0 if kmajor else B0.T) + np.abs(C0)
    assert np.max(np.abs(got - ref) / scale) < 1e-14            # the bound of test_mfma_gemm_matches_numpy


# ------------------------------------------------------------------------------------------------- D-optimal handles
def gaussian(m, n, seed):
    return np.random.RandomState(seed).randn(m, n)


def simplex_point(n, seed):
    x = np.random.RandomState(seed).rand(n) + 0.01
    return x / x.sum()


class Handle:
    """accbpg_dopt_create ... accbpg_dopt_destroy around a block"""

    def __init__(self, lib, V, m, n, ldv, chol_variant=None):
        self.lib, self.h = lib, C.c_void_p()
        ok(lib.accbpg_dopt_create(P(V), m, n, ldv, None, C.byref(self.h), 0), "accbpg_dopt_create")
        if chol_variant is not None:
            ok(lib.accbpg_debug_chol_variant(self.h, chol_variant), "accbpg_debug_chol_variant")

    def __enter__(self):
        return self.h

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.lib.accbpg_dopt_destroy(self.h)
        return False


TWO_LEVEL = 2048 | (1 << 12)            # as test_two_level_cholesky_forced_at_small_sizes
DOPT_SHAPES = [(13, 506, None), (64, 271, None), (65, 267, None), (130, 334, None), (333, 537, None), (520, 723, None),
               (1100, 3000, None), (300, 900, TWO_LEVEL), (256, 1024, None), (64, 65537, None)]
_DOPT_IN = {}


def dopt_inputs(m, n):
    if (m, n) not in _DOPT_IN:
        _DOPT_IN.clear()
        rng = np.random.RandomState(m + n)
        h = {"V": gaussian(m, n, m * 1000 + n), "x": simplex_point(n, m), "x2": simplex_point(n, m + 1),
             "z": simplex_point(n, m + 2), "q": rng.randn(m), "B": rng.randn(m, m)}
        _DOPT_IN[(m, n)] = {k: torch.from_numpy(v).cuda() for k, v in h.items()}
    return _DOPT_IN[(m, n)]


def dopt_case(lib, A, m, n, ldv, xskew, variant):
    d = dopt_inputs(m, n)
    V = A.carve2d(m, n, ldv, data=d["V"], name="V")
    x, x2, z = (A.carve(n, data=d[k], skew=xskew, name=k) for k in ("x", "x2", "z"))
    q = A.carve(m, data=d["q"], name="q")
    B = A.carve2d(m, m, m, data=d["B"], name="B")
    g1, g2, gf, ge, u = (A.carve(n, name=k) for k in ("g_flag1", "g_flag2", "g_factor", "g_eval", "vt_times"))
    # accbpg_dopt_gram writes the lower triangle ("lower triangle significant"): the upper one starts as zeros here, so
    # that the combinations of two Gram matrices hold no sentinel of their inputs
    G1, G2 = (A.carve2d(m, m, m, data=torch.zeros(m, m, dtype=torch.float64), name=k) for k in ("gram1", "gram2"))
    Gc, Ga, Q, Hs = (A.carve2d(m, m, m, name=k) for k in ("lincomb", "lincomb_alias", "Q", "fw_H"))
    c0, c1 = A.carve(m, name="column0"), A.carve(m, name="column_last")
    fx, fw = A.carve(n, name="fw_x"), A.carve(n, name="fw_w")
    ty, tg, tz, tx = (A.carve(n, name=k) for k in ("trial_y", "trial_g", "trial_z", "trial_x"))
    ws = A.carve(lib.accbpg_vec_workspace_doubles(n), name="ws")
    outs = [g1, g2, gf, ge, u, G1, G2, Gc, Ga, Q, Hs, c0, c1, fx, fw, ty, tg, tz, tx]
    A.snapshot()
    res = []
    f = C.c_double()
    with Handle(lib, V, m, n, ldv, variant) as h:
        for flag, g in ((0, None), (1, g1), (2, g2)):
            f.value = 0.0
            ok(lib.accbpg_dopt_func_grad(h, P(x), flag, C.byref(f), P(g)), "func_grad flag %d" % flag)
            res.append(("f_flag%d" % flag, f64(f.value)))
        A.check(writable=[g1, g2], whole=[g1, g2])
        ok(lib.accbpg_dopt_gram(h, P(x), P(G1)), "gram")
        ok(lib.accbpg_dopt_gram(h, P(x2), P(G2)), "gram")
        ok(lib.accbpg_dopt_factor(h, P(G1), C.byref(f)), "factor")
        res.append(("f_factor", f64(f.value)))
        ok(lib.accbpg_dopt_grad(h, P(gf)), "grad")
        ok(lib.accbpg_dopt_eval_gram(h, P(G2), 2, C.byref(f), P(ge)), "eval_gram")
        res.append(("f_eval", f64(f.value)))
        A.check(writable=[g1, g2, G1, G2, gf, ge], whole=[gf, ge])
        ok(lib.accbpg_dopt_gram_lincomb(h, 0.3, P(G1), 0.7, P(G2), P(Gc)), "gram_lincomb")
        Ga.t.copy_(G1.t)
        torch.cuda.synchronize()
        ok(lib.accbpg_dopt_gram_lincomb(h, 0.3, P(Ga), 0.7, P(G2), P(Ga)), "gram_lincomb, out = G1")
        ok(lib.accbpg_dopt_vt_times(h, P(q), P(u)), "vt_times")
        ok(lib.accbpg_dopt_get_column(h, 0, P(c0)), "get_column")
        ok(lib.accbpg_dopt_get_column(h, n - 1, P(c1)), "get_column")
        A.check(writable=[g1, g2, G1, G2, gf, ge, Gc, Ga, u, c0, c1], whole=[Gc, Ga, u, c0, c1])
        ok(lib.accbpg_fw_init(h, P(x), C.byref(f)), "fw_init")
        res.append(("fw_logdet", f64(f.value)))
        ok(lib.accbpg_fw_get_state(h, P(fx), P(fw), P(Hs)), "fw_get_state")
        picked = (C.c_int64 * (2 * m))()
        ok(lib.accbpg_dopt_kyinit(h, P(B), picked, P(Q)), "kyinit")
        res.append(("picked", np.array(list(picked), dtype=np.int64)))
        out = _trial_out()
        rc = lib.accbpg_dopt_burg_trial(h, P(x), P(z), 0.5, 2.0, 1e-8, 0, P(ty), P(tg), P(tz), P(tx), P(ws), C.byref(out))
        ok(rc, "burg_trial")
        res.append(("trial", f64(out.fy, out.lin, out.dxy, out.dzz, out.fx)))
        res.append(("trial_info", np.array(list(out.prox_info), dtype=np.int64)))
    A.check(writable=outs + [ws], whole=[fx, fw, Hs, Q, ty, tg, tz, tx])
    return res + [(v.name, A.bits_of(v)) for v in outs]


def _trial_out():
    from accbpg_and_fw_amd import _lib
    return _lib.TrialOut()


# skewed x: launch_gram picks its kernel by the alignment of x (`xal`) -- the tolerance of
# test_gpu_parity.py::test_gram_unaligned_x_through_c_abi: 1e-11 relative for every scalar and every vector entry on its
# own; the m x m matrices, which that test does not look at, within 1e-11 of their largest entry
_X_SCALARS = ["f_flag0", "f_flag1", "f_flag2", "f_factor", "f_eval", "fw_logdet", "trial"]      # (trial: five scalars)
_X_VECTORS = ["g_flag1", "g_flag2", "g_factor", "g_eval", "fw_x", "fw_w", "trial_y", "trial_g", "trial_z", "trial_x"]
_X_MATRICES = ["gram1", "gram2", "lincomb", "lincomb_alias", "fw_H"]
_X_TOL = dict([(k, ("each", 1e-11)) for k in _X_SCALARS + _X_VECTORS] + [(k, ("norm", 1e-11)) for k in _X_MATRICES])


@pytest.mark.parametrize("xskew", [0, 1])
@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("m,n,variant", DOPT_SHAPES)
def test_dopt_entries(lib, m, n, variant, pad, xskew):
    tol = _X_TOL if xskew else None
    run_case(lambda A: dopt_case(lib, A, m, n, n + pad, xskew, variant), ("dopt", m, n, pad), xskew, tol)


# ------------------------------------------------------------------------------------------------- batches
def batch_case(lib, A, K, m, n, ld, active):
    rng = np.random.RandomState(K * m + n)
    Vs = [A.carve2d(m, n, n, data=gaussian(m, n, 77 * i + m), name="V%d" % i) for i in range(K)]

    def rows(name, fn=None):
        return A.carve2d(K, n, ld, data=None if fn is None else np.stack([fn(i) for i in range(K)]), name=name)

    X = rows("X", lambda i: simplex_point(n, 5 + i))
    Z = rows("Z", lambda i: simplex_point(n, 50 + i))
    Gin = rows("Gin", lambda i: np.random.RandomState(90 + i).randn(n))
    G, Xp, Ax = rows("G"), rows("prox_out"), rows("axpby_out")
    Bm = A.carve(K * m * m, data=rng.randn(K * m * m), name="B")
    Q = A.carve(K * m * m, name="Q")
    st = [(A.carve(n, name="fw_x%d" % i), A.carve(n, name="fw_w%d" % i), A.carve2d(m, m, m, name="fw_H%d" % i))
          for i in range(K)]
    act = (C.c_int * K)(*active)
    on = [i for i in range(K) if active[i]]
    A.snapshot()
    res = []
    b = C.c_void_p()
    ptrs = (C.c_void_p * K)(*[v.ptr for v in Vs])
    ok(lib.accbpg_dopt_batch_create(ptrs, K, m, n, n, None, C.byref(b)), "batch_create")
    try:
        res.append(("fused", np.array([lib.accbpg_dopt_batch_is_fused(b)], dtype=np.int64)))
        f, status = (C.c_double * K)(), (C.c_int * K)()
        ok(lib.accbpg_dopt_batch_func_grad(b, P(X), ld, act, 2, f, P(G), ld, status), "batch_func_grad")
        assert [status[i] for i in on] == [0] * len(on)
        res.append(("f", f64(*[f[i] for i in on])))
        wr = [A.row(G, i) for i in on]
        A.check(writable=wr, whole=wr)
        Ls = (C.c_double * K)(*[1.5 + i for i in range(K)])
        info = (C.c_int * (2 * K))()
        ok(lib.accbpg_dopt_batch_burg_simplex_div_prox(b, P(X), P(Gin), ld, Ls, 1e-8, P(Xp), act, status, info), "batch prox")
        res.append(("prox_info", np.array([info[2 * i + k] for i in on for k in (0, 1)], dtype=np.int64)))
        out = (C.c_double * (3 * K))()
        ok(lib.accbpg_dopt_batch_ls_terms(b, P(Gin), P(X), P(Z), P(Z), P(X), ld, act, out, status), "batch_ls_terms")
        res.append(("ls_terms", f64(*[out[3 * i + k] for i in on for k in range(3)])))
        av, bv = (C.c_double * K)(*[0.25 + i for i in range(K)]), (C.c_double * K)(*[0.75 - i for i in range(K)])
        ok(lib.accbpg_dopt_batch_axpby(b, av, P(X), bv, P(Z), ld, act, P(Ax)), "batch_axpby")
        wr += [A.row(Xp, i) for i in on] + [A.row(Ax, i) for i in on]
        A.check(writable=wr, whole=wr)
        picked = (C.c_int64 * (K * 2 * m))()
        ok(lib.accbpg_dopt_batch_kyinit(b, P(Bm), picked, P(Q)), "batch_kyinit")         # (all K instances)
        res.append(("picked", np.array(list(picked), dtype=np.int64)))
        A.check(writable=wr + [Q], whole=[Q])
        logdet = (C.c_double * K)()
        ok(lib.accbpg_dopt_batch_fw_init(b, P(X), ld, act, logdet, status), "batch_fw_init")
        res.append(("fw_logdet", f64(*[logdet[i] for i in on])))
        from accbpg_and_fw_amd import _lib
        probes = (_lib.FwProbe * K)()
        ok(lib.accbpg_dopt_batch_fw_probe(b, 0, act, probes), "batch_fw_probe")
        res.append(("probe", f64(*[v for i in on for v in (probes[i].i, probes[i].j, probes[i].w_i, probes[i].w_j)])))
        p, xs, xa, hc, hd = (C.c_int64 * K)(), (C.c_double * K)(), (C.c_double * K)(), (C.c_double * K)(), (C.c_double * K)()
        for i in on:                                                # the Frank-Wolfe step of D_opt_alg.py:75-82
            w_i = probes[i].w_i
            t = (w_i / m - 1.0) / (w_i - 1.0)
            p[i], xs[i], xa[i], hc[i], hd[i] = probes[i].i, 1.0 - t, t, -(t / (1.0 + t * (w_i - 1.0))), 1.0 - t
        ok(lib.accbpg_dopt_batch_fw_update(b, act, p, xs, xa, hc, hd), "batch_fw_update")
        for i in on:
            hi = lib.accbpg_dopt_batch_instance(b, i)
            ok(lib.accbpg_fw_get_state(C.c_void_p(hi), P(st[i][0]), P(st[i][1]), P(st[i][2])), "fw_get_state")
        sv = [v for i in on for v in st[i]]
        A.check(writable=wr + [Q] + sv, whole=sv)
    finally:
        torch.cuda.synchronize()
        lib.accbpg_dopt_batch_destroy(b)
    return res + [(v.name, A.bits_of(v)) for v in (G, Xp, Ax, Q)] + [(v.name, A.bits_of(v)) for v in sv]


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("m,n,fused", [(256, 1024, 1), (96, 640, 0)])
def test_batch_entries(lib, m, n, fused, pad):
    """K = 3 with the middle instance inactive: its rows, like the gaps, belong to nobody."""
    run_case(lambda A: batch_case(lib, A, 3, m, n, n + pad, [1, 0, 1]), ("batch", m, n, pad), 0)
    assert int(_PLAIN[("batch", m, n, pad)][0][1][0]) == fused


# ------------------------------------------------------------------------------------------------- Poisson, KL, SymNMF
def regression_case(lib, A, kind, m, n, lda):
    rng = np.random.RandomState(m * 31 + n)
    Am = A.carve2d(m, n, lda, data=rng.rand(m, n), name="A")
    b = A.carve(m, data=rng.rand(m) + 0.2, name="b")
    x = A.carve(n, data=rng.rand(n) / n + 1e-4, name="x")
    g1, g2, ax = A.carve(n, name="g_flag1"), A.carve(n, name="g_flag2"), A.carve(m, name="Ax")
    A.snapshot()
    create, destroy, func_grad, get_ax = (getattr(lib, "accbpg_%s_%s" % (kind, k))
                                          for k in ("create", "destroy", "func_grad", "get_ax"))
    h = C.c_void_p()
    ok(create(P(Am), m, n, lda, P(b), None, C.byref(h)), kind + "_create")
    res = []
    try:
        f = C.c_double()
        for flag, g in ((0, None), (1, g1), (2, g2)):
            ok(func_grad(h, P(x), flag, C.byref(f), P(g)), kind + "_func_grad")
            if flag != 1:
                res.append(("f_flag%d" % flag, f64(f.value)))
        ok(get_ax(h, P(ax)), kind + "_get_ax")
        A.check(writable=[g1, g2, ax], whole=[g1, g2, ax])
    finally:
        torch.cuda.synchronize()
        destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in (g1, g2, ax)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("m,n", [(37, 51), (5, 4096), (1000, 3), (513, 130)])
@pytest.mark.parametrize("kind", ["poisson", "kldiv"])
def test_regression_entries(lib, kind, m, n, pad):
    run_case(lambda A: regression_case(lib, A, kind, m, n, n + pad), (kind, m, n, pad), 0)


def symnmf_case(lib, A, n, r, ldm):
    rng = np.random.RandomState(n * 7 + r)
    W = rng.rand(n, r)
    M0 = W @ W.T
    M = A.carve2d(n, n, ldm, data=M0, name="M")
    X = A.carve(n * r, data=rng.rand(n, r), name="X")
    g1, g2 = A.carve(n * r, name="G_flag1"), A.carve(n * r, name="G_flag2")
    A.snapshot()
    h = C.c_void_p()
    ok(lib.accbpg_symnmf_create(P(M), n, ldm, r, float(np.linalg.norm(M0)), None, C.byref(h)), "symnmf_create")
    res = []
    try:
        f = C.c_double()
        for flag, g in ((0, None), (1, g1), (2, g2)):
            ok(lib.accbpg_symnmf_func_grad(h, P(X), flag, C.byref(f), P(g)), "symnmf_func_grad")
            if flag != 1:
                res.append(("f_flag%d" % flag, f64(f.value)))
        A.check(writable=[g1, g2], whole=[g1, g2])
    finally:
        torch.cuda.synchronize()
        lib.accbpg_symnmf_destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in (g1, g2)]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("n,r", [(1, 1), (17, 3), (400, 50), (257, 64), (300, 70), (513, 130)])
def test_symnmf_entries(lib, n, r, pad):
    run_case(lambda A: symnmf_case(lib, A, n, r, n + pad), ("symnmf", n, r, pad), 0)
