"""The gradient product's two phases and its carried pipeline (colnorm_phases_body in csrc/dopt_kernels.hip).

Per row block of W = L^-1 the production kernel runs a rectangular phase (every fragment row live, no triangular skip in
the loop) and a diagonal phase (16 k-steps in four groups, the skip a template constant), and the last two k-steps of a
row block load the first two stages of the next one, so the pipeline starts once per workgroup.  Every accumulator still
receives the same MFMAs in the same k order and the column sums are added to in the same order: value and gradient are
the same to the bit as under the development variants 1 (builtin loads), 2 (dealt out) and 3 (the production schedule
before the phases: runtime skip, restart per row block), which share none of the new loop."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


def _problem(m, n, ld=None):
    ld = n if ld is None else ld
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    wide = torch.randn(m, ld, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    return wide[:, :n], x


def _variants_agree(acc, V, x):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    f = acc.DOptimalObj(V)
    base = f.func_grad(x, 2)
    try:
        for variant in (1, 2, 3):
            lib.accbpg_debug_chol_variant(f._h, variant << 30)
            fv, g = f.func_grad(x, 2)
            assert fv == base[0], variant
            assert torch.equal(g, base[1]), variant
    finally:
        lib.accbpg_debug_chol_variant(f._h, 0)
    again = f.func_grad(x, 2)
    assert again[0] == base[0] and torch.equal(again[1], base[1])
    return base


def _column_range_agrees(m, n, own_copy):
    """The smallest shapes that reach each seam of the loop have fewer columns than rows (one workgroup is 128
    columns, three row blocks are 768 rows), and a D-optimal objective of their own does not exist for them (V X V^T is
    singular for n < m; DOptimalObj asserts m < n).  They are evaluated the way a column shard of a larger instance is
    (config 5): the handle is a shard handle over n columns of an (m, 2m) matrix, the Gram matrix is
    that of the whole matrix, and accbpg_dopt_eval_gram factors it and forms the shard's gradient with the kernel under
    test.  Value and gradient under variants 1, 2, 3 against production, on one handle."""
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
            res = {}
            for variant in (0, 1, 2, 3):
                lib.accbpg_debug_chol_variant(hs, variant << 30)
                g = torch.empty(n, dtype=torch.float64, device="cuda")
                fv = C.c_double()
                _lib.check(lib.accbpg_dopt_eval_gram(hs, C.c_void_p(gram.data_ptr()), 2, C.byref(fv), C.c_void_p(g.data_ptr())),
                           "accbpg_dopt_eval_gram")
                torch.cuda.synchronize()
                res[variant] = (fv.value, g)
            lib.accbpg_debug_chol_variant(hs, 0)
            for variant in (1, 2, 3):
                assert res[variant][0] == res[0][0], variant
                assert torch.equal(res[variant][1], res[0][1]), variant
            # the shard handle does run the direct-to-LDS gradient kernel (the timing entry refuses any other handle)
            ms = C.c_double()
            scratch = torch.empty(n, dtype=torch.float64, device="cuda")
            assert lib.accbpg_debug_grad_variant(hs, C.c_void_p(scratch.data_ptr()), 0, 1, C.byref(ms)) == 0
            assert torch.equal(scratch, res[0][1])
            assert bool(torch.isfinite(res[0][1]).all()) and bool((res[0][1] < 0).all())
        finally:
            lib.accbpg_dopt_destroy(hs)
    finally:
        lib.accbpg_dopt_destroy(hw)


# (768,128): one workgroup, three row blocks -- row block 0 is diagonal-only, the boundaries 0->1 and 1->2 carry
# prefetched stages, the last block has no successor; (768,256), (1024,384): more than one workgroup, and (1024) a fourth
# row block with 48 rectangular steps
@pytest.mark.parametrize("shape", [(768, 128), (768, 256), (1024, 384)])
def test_phases_are_bit_identical_to_the_variants(acc, shape):
    m, n = shape
    _column_range_agrees(m, n, own_copy=True)


def test_phases_on_a_column_range_of_a_wider_matrix(acc):
    """(1024, 256) read in place as a column range of the (1024, 2048) matrix: ldv != n, rows still 16-byte aligned."""
    _column_range_agrees(1024, 256, own_copy=False)


# (256, 512) is the smallest shape a batch runs fused: one row block, so it guards the batch plumbing only; (768, 2048)
# takes the batch kernel through rectangular phases and carried row-block boundaries as well
@pytest.mark.parametrize("shape", [(256, 512), (768, 2048)])
def test_phases_in_a_lockstep_batch(acc, shape):
    """colnorm_glds_batch_kernel calls the same body: each instance's gradient is bit-identical to that instance
    evaluated alone on a handle with the batch's plan, under production and under the loop as it was (variant 3; the
    batch kernel has no variants, so this compares the new body in the batch against the old one outside it)."""
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.batched import DOptimalBatch
    lib = _lib.load()
    (m, n), K = shape, 2
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
        finally:
            lib.accbpg_debug_chol_variant(inst._h, 0)


def test_phases_against_torch_linalg(acc):
    """All variants could be wrong together: g = -colsum((L^-1 V)^2) with torch.linalg in fp64, rtol 1e-11 (the
    tolerance of the gradient in the parity tests)."""
    m, n = 1024, 4096
    V, x = _problem(m, n)
    fv, g = _variants_agree(acc, V, x)
    Vc, xc = V.cpu(), x.cpu()
    L = torch.linalg.cholesky((Vc * xc) @ Vc.T)
    Y = torch.linalg.solve_triangular(L, Vc, upper=False)
    ref = -(Y * Y).sum(0)
    err = ((g.cpu() - ref).abs() / ref.abs()).max().item()
    print("max relative error of the gradient against torch.linalg: %.3e" % err)
    np.testing.assert_allclose(g.cpu().numpy(), ref.numpy(), rtol=1e-11, atol=0.0)
    assert abs(fv - (-2.0 * torch.log(torch.diagonal(L)).sum().item())) < 1e-11 * abs(fv)
