"""The gradient product's k-step, dealt out (Tile::grad_step_dealt in csrc/mfma_tile.hpp).

Production deals the fragment reads and the loads of a k-step out behind pairs of MFMAs in every rectangular step and in
diagonal steps 0..4; the loop it replaces ran them as blocks at the fragment-group boundaries and is still there, launched
by accbpg_debug_grad_variant code 4 (code 5: the dealt-out placement production does not use, code 6: only the rectangular
steps dealt out).  Every accumulator receives the same MFMAs in the same k order under all four, so the gradient has the
same bits, and the value (which the gradient kernel does not enter) is what it
was.  The shapes are the smallest that reach each seam of the loop.  From m = 768 on they have fewer columns than rows and
are evaluated the way a column shard of a larger instance is (tests/test_gpu_grad_phases.py: _column_range_agrees).  Below
m = 768 a handle of its own takes the 64 x 64 tile and never reaches this kernel (accbpg_debug_grad_variant refuses it); the
256 x 128 tile runs there for the instances of a lock-step batch only, so one and two row blocks are instances of a batch at
the smallest width a batch runs fused."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# accbpg_debug_grad_variant: every k-step on the block schedule / the other placement / only the rectangular steps dealt out
BLOCK, OTHER, RECT_ONLY = 4, 5, 6


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _problem(m, n):
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    return V, x


def _variant_gradient(lib, h, n, code):
    g = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    ms = C.c_double()
    assert lib.accbpg_debug_grad_variant(h, C.c_void_p(g.data_ptr()), code, 1, C.byref(ms)) == 0, code
    torch.cuda.synchronize()
    return g


def _column_range_agrees(m, n, own_copy):
    """A shard handle over n columns of an (m, 2m) matrix: the Gram matrix is that of the whole matrix,
    accbpg_dopt_eval_gram factors it and forms the shard's gradient with the production kernel.  The loop before this
    change and the other placement then read the same inverse factor on the same handle."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    nw = 2 * m
    V, x = _problem(m, nw)
    Vs = V[:, :n].contiguous() if own_copy else V[:, :n]
    ld = Vs.stride(0)
    assert ld == (n if own_copy else nw) and Vs.data_ptr() % 16 == 0 and (ld * 8) % 16 == 0
    hw, hs = C.c_void_p(), C.c_void_p()
    _lib.check(lib.accbpg_dopt_create(C.c_void_p(V.data_ptr()), m, nw, nw, None, C.byref(hw), 0), "accbpg_dopt_create")
    try:
        _lib.check(lib.accbpg_dopt_create(C.c_void_p(Vs.data_ptr()), m, n, ld, None, C.byref(hs), 1), "accbpg_dopt_create")
        try:
            gram = torch.empty(m, m, dtype=torch.float64, device="cuda")
            _lib.check(lib.accbpg_dopt_gram(hw, C.c_void_p(x.data_ptr()), C.c_void_p(gram.data_ptr())), "accbpg_dopt_gram")
            torch.cuda.synchronize()

            def evaluate():
                g = torch.empty(n, dtype=torch.float64, device="cuda")
                fv = C.c_double()
                _lib.check(lib.accbpg_dopt_eval_gram(hs, C.c_void_p(gram.data_ptr()), 2, C.byref(fv), C.c_void_p(g.data_ptr())),
                           "accbpg_dopt_eval_gram")
                torch.cuda.synchronize()
                return torch.tensor(fv.value, dtype=torch.float64), g

            fv, g = evaluate()
            assert bool(torch.isfinite(g).all()) and bool((g < 0).all())
            for code in (0, BLOCK, OTHER, RECT_ONLY):
                assert torch.equal(_variant_gradient(lib, hs, n, code), g), code
            # the handle is what it was: value and gradient once more
            fv2, g2 = evaluate()
            assert torch.equal(fv2, fv) and torch.equal(g2, g)
        finally:
            lib.accbpg_dopt_destroy(hs)
    finally:
        lib.accbpg_dopt_destroy(hw)


def _batch_agrees(m, n, K=2):
    """colnorm_glds_batch_kernel calls the same body with the production schedule: each instance's gradient is
    bit-identical to that instance evaluated alone under variant 3 of the handle's switch (the loop before the phases,
    which shares nothing with the new step), and to the block schedule, the other placement and the rectangular-only
    dealing on the instance's own inverse factor."""
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.batched import DOptimalBatch
    lib = _lib.load()
    gen = torch.Generator(device="cuda").manual_seed(77 + m)
    Vs = [torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(K)]
    X = torch.rand(K, n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    X /= X.sum(1, keepdim=True)
    batch = DOptimalBatch(Vs)
    assert batch.fused
    f, G = batch.func_grad(X, 2)
    for i in range(K):
        inst = batch.instance(i)
        try:
            for variant in (0, 3):
                lib.accbpg_debug_chol_variant(inst._h, variant << 30)
                fi, gi = inst.func_grad(X[i], 2)
                assert f[i] == fi, (i, variant)
                assert torch.equal(G[i], gi), (i, variant)
            for code in (0, BLOCK, OTHER, RECT_ONLY):
                assert torch.equal(_variant_gradient(lib, inst._h, n, code), G[i]), (i, code)
        finally:
            lib.accbpg_debug_chol_variant(inst._h, 0)


# m = 256: one row block, diagonal phase only; m = 512: the first rectangular phase (16 steps) and one carried boundary
@pytest.mark.parametrize("shape", [(256, 512), (512, 1024)])
def test_dealt_step_below_three_row_blocks(acc, shape):
    _batch_agrees(*shape)


def test_dealt_step_is_bit_identical_to_the_block_schedule(acc):
    """(768,256): two workgroups, rectangular phases of 16 and 32 steps, the last block without a successor."""
    _column_range_agrees(768, 256, own_copy=True)


def test_dealt_step_on_a_column_range_of_a_wider_matrix(acc):
    """(1024, 256) read in place as a column range of the (1024, 2048) matrix: ldv != n."""
    _column_range_agrees(1024, 256, own_copy=False)


def test_dealt_step_in_a_lockstep_batch(acc):
    """One lock-step batch of K = 2 at (768, 2048): rectangular phases and carried row-block boundaries in the batch kernel."""
    _batch_agrees(768, 2048)
