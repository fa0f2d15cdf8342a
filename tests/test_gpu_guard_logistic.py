"""Guard bands around the caller's buffers of the accbpg_logistic_* entry points and of the L2L1Linf vector entries
(tests/guard_arena.py): A (with gap columns where lda > n), y, x, the gradients of flags 1 and 2, the three outputs of
accbpg_logistic_get, the output of accbpg_l2l1linf_prox and the inputs and the workspace of accbpg_l1_norm and
accbpg_sq_ls_terms are carved out of one arena filled with a sentinel; no double outside the named outputs may change,
the outputs must be written whole, and every result must have the bits of the same calls on plain allocations.
Shapes: both forms of the A x pass, one and several row splits of the A^T r pass, odd n, odd and even lda, x at 16
bytes and at 8 mod 16."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from accbpg_and_fw_amd import _lib
    return _lib.load()


def P(v):
    return C.c_void_p(v.ptr) if v is not None else None


def ok(rc, what):
    from accbpg_and_fw_amd import _lib
    assert rc == 0, "%s returned %d: %s" % (what, rc, _lib.last_error())


def carve_x(A, n, data, skew):
    """x at the asked 16-byte phase in either kind of arena: Plain always hands out 16-byte aligned buffers, and pass 1
    adds a row in another order when x is not, so the plain call gets an x of its own at 8 mod 16"""
    if not (isinstance(A, GA.Plain) and skew):
        return A.carve(n, data=data, skew=skew, name="x")
    buf = torch.zeros(n + 2, dtype=torch.float64, device="cuda")
    off = (1 - buf.data_ptr() // 8) % 2
    t = buf[off:off + n]
    t.copy_(torch.from_numpy(np.ascontiguousarray(data)))
    assert t.data_ptr() % 16 == 8
    return GA.View("x", off, 1, n, n, 0, t)


def logistic_case(lib, A, m, n, lda, skew):
    rng = np.random.RandomState(m * 31 + n)
    Am = A.carve2d(m, n, lda, data=rng.randn(m, n), name="A")
    y = A.carve(m, data=rng.choice([-1.0, 1.0], size=m), name="y")
    x = carve_x(A, n, rng.randn(n) / np.sqrt(n), skew)
    g1, g2 = A.carve(n, name="g_flag1"), A.carve(n, skew=skew, name="g_flag2")
    ax, t, r = A.carve(m, name="Ax"), A.carve(m, skew=skew, name="t"), A.carve(m, name="r")
    A.snapshot()
    h = C.c_void_p()
    ok(lib.accbpg_logistic_create(P(Am), m, n, lda, P(y), None, C.byref(h)), "logistic_create")
    res = []
    try:
        f = (C.c_double * 1)()
        for flag, g in ((0, None), (1, g1), (2, g2)):
            ok(lib.accbpg_logistic_func_grad(h, P(x), flag, f, P(g)), "logistic_func_grad")
            if flag != 1:
                res.append(("f_flag%d" % flag, np.array([f[0]])))
        for which, out in enumerate((ax, t, r)):
            ok(lib.accbpg_logistic_get(h, which, P(out)), "logistic_get")
        A.check(writable=[g1, g2, ax, t, r], whole=[g1, g2, ax, t, r])
    finally:
        torch.cuda.synchronize()
        lib.accbpg_logistic_destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in (g1, g2, ax, t, r)]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("pad", [0, 2, 3])
@pytest.mark.parametrize("m,n", [(37, 51), (5, 4097), (1000, 3), (513, 130), (2050, 64)])
def test_logistic_entries_stay_inside_their_buffers(lib, m, n, pad, skew):
    want = logistic_case(lib, GA.Plain(), m, n, n + pad, skew)
    got = logistic_case(lib, GA.Arena(), m, n, n + pad, skew)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), name


def vector_case(lib, A, n, skew):
    """the prox in both forms, the l1 norm and the line-search terms with and without g and z"""
    rng = np.random.RandomState(n)
    ws_n = int(lib.accbpg_vec_workspace_doubles(n))
    y = A.carve(n, data=rng.randn(n), skew=skew, name="y")
    g = A.carve(n, data=rng.randn(n), name="g")
    z = A.carve(n, data=rng.randn(n), skew=skew, name="z")
    z1 = A.carve(n, data=rng.randn(n), name="z1")
    p1, p2 = A.carve(n, skew=skew, name="prox"), A.carve(n, name="div_prox")
    ws = A.carve(ws_n, name="ws")
    A.snapshot()
    ok(lib.accbpg_l2l1linf_prox(None, P(g), 0.7, 0.2, 1.0, n, P(p1), None), "l2l1linf_prox")
    ok(lib.accbpg_l2l1linf_prox(P(y), P(g), 0.7, 0.2, 1.0, n, P(p2), None), "l2l1linf_prox (div)")
    res = []
    o1, o3 = C.c_double(0.0), (C.c_double * 3)()
    ok(lib.accbpg_l1_norm(P(y), n, C.byref(o1), P(ws), None), "l1_norm")
    res.append(("l1", np.array([o1.value])))
    for name, gg, zz, zz1 in (("ls", g, z, z1), ("ls_no_g", None, z, z1), ("ls_no_z", g, None, None)):
        ok(lib.accbpg_sq_ls_terms(P(gg), P(p1), P(y), P(zz), P(zz1), n, o3, P(ws), None), name)
        res.append((name, np.array(list(o3))))
    A.check(writable=[p1, p2, ws], whole=[p1, p2])
    return res + [(v.name, A.bits_of(v)) for v in (p1, p2)]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 1025, 4097, 300001])
def test_vector_entries_stay_inside_their_buffers(lib, n, skew):
    want = vector_case(lib, GA.Plain(), n, skew)
    got = vector_case(lib, GA.Arena(), n, skew)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        assert np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64)), name


def test_bad_arguments_are_refused(lib):
    A = GA.Plain()
    Am = A.carve2d(4, 3, 3, data=np.ones((4, 3)), name="A")
    y, x, g, out = A.carve(4, data=np.ones(4)), A.carve(3, data=np.ones(3)), A.carve(3), A.carve(4)
    ws = A.carve(int(lib.accbpg_vec_workspace_doubles(3)))
    h = C.c_void_p()
    assert lib.accbpg_logistic_create(P(Am), 4, 3, 2, P(y), None, C.byref(h)) == 4      # lda < n
    assert lib.accbpg_logistic_create(None, 4, 3, 3, P(y), None, C.byref(h)) == 4
    assert lib.accbpg_logistic_create(P(Am), 4, 3, 3, None, None, C.byref(h)) == 4
    ok(lib.accbpg_logistic_create(P(Am), 4, 3, 3, P(y), None, C.byref(h)), "logistic_create")
    f = (C.c_double * 1)()
    assert lib.accbpg_logistic_func_grad(h, P(x), 3, f, P(g)) == 4
    assert lib.accbpg_logistic_func_grad(h, P(x), -1, f, P(g)) == 4
    assert lib.accbpg_logistic_func_grad(h, P(x), 2, None, P(g)) == 4
    assert lib.accbpg_logistic_func_grad(h, P(x), 1, f, None) == 4
    assert lib.accbpg_logistic_func_grad(h, P(x), 1, f, P(x)) == 4                       # g must not be x
    assert lib.accbpg_logistic_func_grad(h, None, 0, f, None) == 4
    assert lib.accbpg_logistic_get(h, 0, None) == 4 and lib.accbpg_logistic_get(h, 3, P(out)) == 4
    assert lib.accbpg_logistic_set_stream(None, None) == 4
    assert lib.accbpg_logistic_destroy(h) == 0 and lib.accbpg_logistic_destroy(None) == 0
    o = (C.c_double * 3)()
    assert lib.accbpg_l2l1linf_prox(None, None, 1.0, 0.1, 1.0, 3, P(g), None) == 4
    assert lib.accbpg_l2l1linf_prox(None, P(x), 0.0, 0.1, 1.0, 3, P(g), None) == 1      # L must be positive
    assert lib.accbpg_l1_norm(None, 3, o, P(ws), None) == 4 and lib.accbpg_l1_norm(P(x), 3, o, None, None) == 4
    assert lib.accbpg_sq_ls_terms(None, P(x), P(x), P(x), None, 3, o, P(ws), None) == 4  # z without z1
    assert lib.accbpg_sq_ls_terms(None, None, P(x), None, None, 3, o, P(ws), None) == 4
