"""The chain workgroups of the one-launch Cholesky at the sizes where their panel solve first changes behaviour.

The chain workgroup of block row d looks for its diagonal tile's hand-over (from the owner of tile (d,0)) beside every look
for a piece of the factor, and runs the update of the columns to the right of a solved panel with the blocks of a wave
interleaved.  T = 3 (m = 130, 192) is the first size with such a hand-over (d = 2); T = 4 … 6 with ragged last blocks
follow.  test_tile_cholesky_matches_step_kernels covers none of these sizes.

Everything here is `==` / array_equal: the launch-per-column kernels and the bits recorded from the parent commit
(tests/golden/chol_pace_parent.npz, written by tools/gen_chol_pace_golden.py) are both exact references."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN, gaussian_design

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SHAPES = [130, 192, 200, 256, 320, 333]


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def lib(acc):
    from accbpg_and_fw_amd import _lib
    return _lib.load()


@pytest.fixture(scope="module")
def parent():
    return np.load(os.path.join(GOLDEN, "chol_pace_parent.npz"), allow_pickle=False)


def _instance(m):
    n = m + 200 + (m % 7)
    V = gaussian_design(m, n, 40 + m % 13)
    rng = np.random.RandomState(m)
    x = rng.rand(n) + 0.01
    x /= x.sum()
    return n, V, x


def _fresh(acc, lib, V, variant=0):
    f = acc.DOptimalObj(V)
    lib.accbpg_dopt_value_reuse(f._h, 0)                    # every evaluation runs its own factorisation
    if variant:
        assert lib.accbpg_debug_chol_variant(f._h, variant) == 0
    return f


@pytest.mark.parametrize("m", SHAPES)
def test_chain_matches_step_kernels_and_parent(acc, lib, parent, m):
    """(a) value-only (no inverse blocks) and func_grad(x, 2) of the one-launch path against the launch-per-column
    kernels; (b) both against the bits of the parent commit."""
    n, V, x = _instance(m)
    assert int(parent["n_%d" % m]) == n and int(parent["seed_v_%d" % m]) == 40 + m % 13 and int(parent["seed_x_%d" % m]) == m
    f_tiles = _fresh(acc, lib, V)
    f_steps = _fresh(acc, lib, V, 64)                       # bit 6: launch per block column
    va = f_tiles(x)
    vb = f_steps(x)
    a, ga = f_tiles.func_grad(x, 2)
    b, gb = f_steps.func_grad(x, 2)
    assert va == vb
    assert a == b
    np.testing.assert_array_equal(ga, gb)
    assert va == float(parent["f_value_%d" % m])
    assert a == float(parent["f_%d" % m])
    np.testing.assert_array_equal(ga, parent["g_%d" % m])


@pytest.mark.parametrize("shape", [(320, 525), (2048, 4096)])
def test_repeats_beside_a_second_stream_are_bit_identical(acc, lib, shape):
    """(c) 40 func_grad(x, 2) on one handle while a second handle on a second stream runs value evaluations beside them:
    the looks ahead (pieces and the diagonal tile) see uneven load and a warm L1; every result equals the first."""
    m, n = shape
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    x2 = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x2 /= x2.sum()
    f1 = _fresh(acc, lib, V)
    f2 = _fresh(acc, lib, V)
    side = torch.cuda.Stream()
    assert lib.accbpg_dopt_set_stream(f2._h, C.c_void_p(side.cuda_stream)) == 0
    torch.cuda.synchronize()
    first = None
    v2 = C.c_double(0.0)
    for it in range(40):
        assert lib.accbpg_dopt_func_grad_begin(f2._h, C.c_void_p(x2.data_ptr()), 0, None) == 0
        fv, g = f1.func_grad(x, 2)
        assert lib.accbpg_dopt_func_grad_end(f2._h, C.byref(v2)) == 0
        if first is None:
            first = (fv, g.clone(), v2.value)
            continue
        assert fv == first[0], it
        assert torch.equal(g, first[1]), it
        assert v2.value == first[2], it
    torch.cuda.synchronize()
    assert np.isfinite(first[0]) and np.isfinite(first[2])


def test_abandoned_launch_still_redoes(acc, lib, parent):
    """The stall switch (block column 0 never published, 2 ms spin limit) once at m = 320: the launch is abandoned from
    inside the chain's waits -- the look for the diagonal tile included -- and the redo returns the parent's value."""
    m = 320
    n, V, x = _instance(m)
    g = _fresh(acc, lib, V, 128)                            # bit 7: stall + 2 ms spin limit
    got = g.func_grad(x, 2)
    assert got[0] == float(parent["f_%d" % m])
    np.testing.assert_array_equal(got[1], parent["g_%d" % m])
