"""Guard bands around the caller's buffers of the accbpg_svm_* entry points (tests/guard_arena.py): A (with gap columns
where lda > n), y, x, the gradients of flags 1, 2 and 3 and the output of accbpg_svm_get_ax are carved out of one
arena filled with a sentinel; no double outside the named outputs may change, the outputs must be written whole, and
every result must have the bits of the same calls on plain allocations.  Shapes: both forms of the A x pass, one and
several row splits of the A^T r pass, odd n, odd and even lda, x at 16 bytes and at 8 mod 16."""
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


def svm_case(lib, A, m, n, lda, skew):
    rng = np.random.RandomState(m * 31 + n)
    Am = A.carve2d(m, n, lda, data=rng.randn(m, n), name="A")
    y = A.carve(m, data=rng.choice([-1.0, 1.0], size=m), name="y")
    x = A.carve(n, data=rng.randn(n) / np.sqrt(n), skew=skew, name="x")
    g1, g2, g3 = A.carve(n, name="g_flag1"), A.carve(n, skew=skew, name="g_flag2"), A.carve(n, name="g_flag3")
    ax = A.carve(m, name="Ax")
    A.snapshot()
    h = C.c_void_p()
    ok(lib.accbpg_svm_create(P(Am), m, n, lda, P(y), None, C.byref(h)), "svm_create")
    res = []
    try:
        f = (C.c_double * 2)()
        for flag, g in ((0, None), (1, g1), (2, g2), (3, g3)):
            ok(lib.accbpg_svm_func_grad(h, P(x), 0.3, flag, f, P(g)), "svm_func_grad")
            if flag in (0, 2):
                res.append(("f_flag%d" % flag, np.array([f[0], f[1]])))
        ok(lib.accbpg_svm_get_ax(h, P(ax)), "svm_get_ax")
        A.check(writable=[g1, g2, g3, ax], whole=[g1, g2, g3, ax])
    finally:
        torch.cuda.synchronize()
        lib.accbpg_svm_destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in (g1, g2, g3, ax)]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("pad", [0, 2, 3])
@pytest.mark.parametrize("m,n", [(37, 51), (5, 4097), (1000, 3), (513, 130), (2050, 64)])
def test_svm_entries_stay_inside_their_buffers(lib, m, n, pad, skew):
    want = svm_case(lib, GA.Plain(), m, n, n + pad, skew)
    got = svm_case(lib, GA.Arena(), m, n, n + pad, skew)
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, name
        if skew == 0:
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), name
        else:
            # the plain x lies on 16 bytes and the carved one does not: pass 1 adds each row in another order
            a, b = a.view(np.float64), b.view(np.float64)
            assert np.all(np.abs(a - b) <= 1e-12 * np.max(np.abs(b))), name


def test_bad_arguments_are_refused(lib):
    A = GA.Plain()
    Am = A.carve2d(4, 3, 3, data=np.ones((4, 3)), name="A")
    y, x, g = A.carve(4, data=np.ones(4)), A.carve(3, data=np.ones(3)), A.carve(3)
    h = C.c_void_p()
    assert lib.accbpg_svm_create(P(Am), 4, 3, 2, P(y), None, C.byref(h)) == 4          # lda < n
    assert lib.accbpg_svm_create(None, 4, 3, 3, P(y), None, C.byref(h)) == 4
    ok(lib.accbpg_svm_create(P(Am), 4, 3, 3, P(y), None, C.byref(h)), "svm_create")
    f = (C.c_double * 2)()
    assert lib.accbpg_svm_func_grad(h, P(x), 0.1, 4, f, P(g)) == 4
    assert lib.accbpg_svm_func_grad(h, P(x), 0.1, 2, None, P(g)) == 4
    assert lib.accbpg_svm_func_grad(h, P(x), 0.1, 1, f, None) == 4
    assert lib.accbpg_svm_func_grad(h, P(x), 0.1, 1, f, P(x)) == 4                      # g must not be x
    assert lib.accbpg_svm_get_ax(h, None) == 4
    assert lib.accbpg_svm_destroy(h) == 0 and lib.accbpg_svm_destroy(None) == 0
