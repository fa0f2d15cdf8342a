"""Guard bands around the device operands of ``accbpg_dopt_batch_burg_simplex_avg_prox`` (tests/guard_arena.py, as
tests/test_gpu_guard_caller.py has them for the other batch entries): the design matrices, both inputs and both outputs
are carved out of one sentinel-filled arena, K = 3 with the middle instance inactive.  Behind the call no double
outside the gavg_out and z_out rows of the active instances has changed -- bands, the gap columns [n, ld), the inactive
rows and the inputs alike --, those rows hold no sentinel any more, and every result equals that of the same call on
plain tensors bit for bit.  Sizes: one past each seam of the registers-per-thread dispatch, 32769 being the first row
that runs the sequential composition through the batch's scratch."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guard_arena as GA  # noqa: E402

pytestmark = pytest.mark.gpu

K, M = 3, 8
ACTIVE = [1, 0, 1]


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from accbpg_and_fw_amd import _lib
    return _lib.load()


def P(v):
    return C.c_void_p(v.ptr)


def case(lib, A, n, ld):
    rng = np.random.RandomState(n)
    Vs = [A.carve2d(M, n, n, data=np.random.RandomState(77 * i + M).randn(M, n), name="V%d" % i) for i in range(K)]
    Gavg = A.carve2d(K, n, ld, data=5.0 * rng.randn(K, n), name="gavg")
    G = A.carve2d(K, n, ld, data=3.0 * rng.randn(K, n), name="g")
    Gout = A.carve2d(K, n, ld, name="gavg_out")
    Z = A.carve2d(K, n, ld, name="z_out")
    wgt = (C.c_double * K)(1.75, 2.5, 3.25)
    csum = (C.c_double * K)(2.75, 4.0, 7.5)
    Lc = (C.c_double * K)(*[1.0 / csum[i] for i in range(K)])
    act = (C.c_int * K)(*ACTIVE)
    on = [i for i in range(K) if ACTIVE[i]]
    A.snapshot()
    b = C.c_void_p()
    ptrs = (C.c_void_p * K)(*[v.ptr for v in Vs])
    assert lib.accbpg_dopt_batch_create(ptrs, K, M, n, n, None, C.byref(b)) == 0
    try:
        status, info = (C.c_int * K)(), (C.c_int * (2 * K))()
        rc = lib.accbpg_dopt_batch_burg_simplex_avg_prox(b, P(Gavg), P(G), ld, wgt, csum, Lc, 1e-8, P(Gout), P(Z), act,
                                                         status, info)
        assert rc == 0 and [status[i] for i in on] == [0] * len(on)
        wr = [A.row(Gout, i) for i in on] + [A.row(Z, i) for i in on]
        A.check(writable=wr, whole=wr)
    finally:
        torch.cuda.synchronize()
        lib.accbpg_dopt_batch_destroy(b)
    return [("info", np.array([info[2 * i + k] for i in on for k in (0, 1)], dtype=np.int64)),
            ("gavg_out", A.bits_of(Gout)), ("z_out", A.bits_of(Z))]


@pytest.mark.parametrize("pad", [0, 5])
@pytest.mark.parametrize("n", [1025, 8193, 32769])
def test_avg_prox_writes_only_the_active_output_rows(lib, n, pad):
    want = case(lib, GA.Plain(), n, n + pad)
    got = case(lib, GA.Arena(), n, n + pad)
    for (name, a), (_, b) in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a, b), name
