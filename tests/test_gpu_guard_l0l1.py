"""Guard bands around the caller's buffers of accbpg_fw_direction and of the four accbpg_logistic_line_* /
func_grad_carried entries (tests/guard_arena.py), on the model of tests/test_gpu_guard_logistic.py: g, x, the centre, s,
d and the workspace of the direction step, and A (with gap columns where lda > n), y, x, d and the gradient of the
carried func_grad are carved out of one arena filled with a sentinel; no double outside the named outputs may change,
the outputs must be written whole, and every result must have the bits of the same calls on plain allocations."""
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


def same(got, want):
    assert [k for k, _ in got] == [k for k, _ in want]
    for (name, a), (_, b) in zip(got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, name
        assert np.array_equal(a.view(np.int64), b.view(np.int64)), name


def direction_case(lib, A, n, skew):
    """the three oracles, the balls with a scalar and an array centre"""
    rng = np.random.RandomState(n)
    g = A.carve(n, data=rng.randn(n), skew=skew, name="g")
    x = A.carve(n, data=0.3 * rng.randn(n), name="x")
    c = A.carve(n, data=0.5 * rng.randn(n), skew=skew, name="c")
    outs = [(A.carve(n, skew=skew, name="s%d" % i), A.carve(n, name="d%d" % i)) for i in range(5)]
    ws = A.carve(int(lib.accbpg_vec_workspace_doubles(n)), name="ws")
    A.snapshot()
    res = []
    calls = ((0, 0, None, 0.25), (0, 1, c, 0.0), (1, 0, None, 0.0), (1, 1, c, 0.0), (2, 0, None, 0.0))
    for (lmo, kind, cen, val), (s, d) in zip(calls, outs):
        o5, idx = (C.c_double * 5)(), (C.c_int64 * 1)()
        ok(lib.accbpg_fw_direction(P(g), P(x), lmo, kind, P(cen), val, 1.5, n, P(s), P(d), o5, idx, P(ws), None),
           "fw_direction")
        res.append(("sums %d %d" % (lmo, kind), np.array(list(o5))))
        res.append(("idx %d %d" % (lmo, kind), np.array([float(idx[0])])))
    flat = [v for pair in outs for v in pair]
    A.check(writable=flat + [ws], whole=flat)
    return res + [(v.name, A.bits_of(v)) for v in flat]


@pytest.mark.parametrize("skew", [0, 1])
@pytest.mark.parametrize("n", [1, 65, 1025, 4097, 300001])
def test_direction_stays_inside_its_buffers(lib, n, skew):
    same(direction_case(lib, GA.Arena(), n, skew), direction_case(lib, GA.Plain(), n, skew))


def line_case(lib, A, m, n, lda):
    rng = np.random.RandomState(m * 31 + n)
    Am = A.carve2d(m, n, lda, data=rng.randn(m, n), name="A")
    y = A.carve(m, data=rng.choice([-1.0, 1.0], size=m), name="y")
    x = A.carve(n, data=rng.randn(n) / np.sqrt(n), name="x")
    d = A.carve(n, data=rng.randn(n) / np.sqrt(n), name="d")
    g0, g1, g2 = A.carve(n, name="g"), A.carve(n, name="g_carried1"), A.carve(n, name="g_carried2")
    ax, t, r = A.carve(m, name="Ax"), A.carve(m, name="t"), A.carve(m, name="r")
    A.snapshot()
    h = C.c_void_p()
    ok(lib.accbpg_logistic_create(P(Am), m, n, lda, P(y), None, C.byref(h)), "logistic_create")
    res = []
    try:
        f = (C.c_double * 1)()
        ok(lib.accbpg_logistic_func_grad(h, P(x), 2, f, P(g0)), "logistic_func_grad")
        ok(lib.accbpg_logistic_line_begin(h, P(d)), "line_begin")
        for a in (1.0, 0.25):
            ok(lib.accbpg_logistic_line_value(h, a, f), "line_value")
            res.append(("value %g" % a, np.array([f[0]])))
        ok(lib.accbpg_logistic_line_accept(h, 0.25), "line_accept")
        ok(lib.accbpg_logistic_func_grad_carried(h, 1, f, P(g1)), "func_grad_carried 1")
        ok(lib.accbpg_logistic_func_grad_carried(h, 2, f, P(g2)), "func_grad_carried 2")
        res.append(("carried value", np.array([f[0]])))
        ok(lib.accbpg_logistic_func_grad_carried(h, 0, f, None), "func_grad_carried 0")
        res.append(("carried value, flag 0", np.array([f[0]])))
        for which, out in enumerate((ax, t, r)):
            ok(lib.accbpg_logistic_get(h, which, P(out)), "logistic_get")
        outs = [g0, g1, g2, ax, t, r]
        A.check(writable=outs, whole=outs)
    finally:
        torch.cuda.synchronize()
        lib.accbpg_logistic_destroy(h)
    return res + [(v.name, A.bits_of(v)) for v in outs]


@pytest.mark.parametrize("pad", [0, 2, 3])
@pytest.mark.parametrize("m,n", [(37, 51), (5, 4097), (1000, 3), (2050, 64)])
def test_line_entries_stay_inside_their_buffers(lib, m, n, pad):
    same(line_case(lib, GA.Arena(), m, n, n + pad), line_case(lib, GA.Plain(), m, n, n + pad))


def test_bad_arguments_are_refused(lib):
    A = GA.Plain()
    Am = A.carve2d(4, 3, 3, data=np.ones((4, 3)), name="A")
    y, x, g = A.carve(4, data=np.ones(4)), A.carve(3, data=np.ones(3)), A.carve(3)
    s, d = A.carve(3), A.carve(3)
    ws = A.carve(int(lib.accbpg_vec_workspace_doubles(3)))
    o5, idx, f = (C.c_double * 5)(), (C.c_int64 * 1)(), (C.c_double * 1)()
    args = lambda **k: [k.get("g", P(x)), k.get("x", P(x)), k.get("lmo", 0), k.get("kind", 0), k.get("c", None), 0.0, 1.0,
                        k.get("n", 3), k.get("s", P(s)), k.get("d", P(d)), k.get("o", o5), idx, k.get("ws", P(ws)), None]
    assert lib.accbpg_fw_direction(*args()) == 0
    for bad in (dict(g=None), dict(x=None), dict(s=None), dict(d=None), dict(o=None), dict(ws=None), dict(n=0),
                dict(lmo=3), dict(lmo=-1), dict(kind=2), dict(kind=1), dict(s=P(d)), dict(s=P(x)), dict(d=P(x))):
        assert lib.accbpg_fw_direction(*args(**bad)) == 4, bad
    assert lib.accbpg_fw_direction(*args(lmo=2, kind=1)) == 0              # the simplex ignores the centre
    h = C.c_void_p()
    ok(lib.accbpg_logistic_create(P(Am), 4, 3, 3, P(y), None, C.byref(h)), "logistic_create")
    assert lib.accbpg_logistic_line_begin(h, P(x)) == 4                     # stale: no func_grad yet
    assert lib.accbpg_logistic_func_grad_carried(h, 0, f, None) == 4
    ok(lib.accbpg_logistic_func_grad(h, P(x), 0, f, None), "func_grad")
    assert lib.accbpg_logistic_line_value(h, 0.5, f) == 4 and lib.accbpg_logistic_line_accept(h, 0.5) == 4
    assert lib.accbpg_logistic_line_begin(h, None) == 4 and lib.accbpg_logistic_line_begin(None, P(x)) == 4
    ok(lib.accbpg_logistic_line_begin(h, P(x)), "line_begin")
    assert lib.accbpg_logistic_line_value(h, 0.5, None) == 4 and lib.accbpg_logistic_line_value(None, 0.5, f) == 4
    assert lib.accbpg_logistic_line_accept(None, 0.5) == 4
    assert lib.accbpg_logistic_func_grad_carried(h, 3, f, P(g)) == 4
    assert lib.accbpg_logistic_func_grad_carried(h, 1, f, None) == 4
    assert lib.accbpg_logistic_func_grad_carried(h, 2, None, P(g)) == 4
    assert lib.accbpg_logistic_func_grad_carried(None, 0, f, None) == 4
    ok(lib.accbpg_logistic_line_value(h, 0.5, f), "line_value")
    torch.cuda.synchronize()
    assert lib.accbpg_logistic_destroy(h) == 0
