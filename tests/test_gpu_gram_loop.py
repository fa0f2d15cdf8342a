"""The Gram kernel's k-loop with the stage as a compile-time constant (gram_streamk_glds_body, GV & 512) against the
loop rolled over a runtime stage index that production ran before (bit 10 of accbpg_debug_chol_variant puts it back
under schedule 0; accbpg_debug_gram_variant times the two as codes 30 and 28).

Every accumulator receives the same MFMAs on the same operands in the same k order under both, so the Gram matrix, the
value and the gradient have the same bits -- also against schedule 3 (the block schedule), which shares no loop code with
either.  What can go wrong in the new loop is its control flow: a segment of L k-steps runs (max(L - 2, 0)) / 3 trips of
three steps and a tail of one to four, the tail sets its load sources step by step, and every segment restarts the
pipeline at stage 0.  So the shapes are chosen from the plan (csrc/dopt_plan.hpp compiles alone, as in
tests/test_plan_cpu.py) and each test asserts that its shapes have the segments it is there for.  A wrong stage, a wrong
fragment address or a wrong source shows as wrong data; on integer-valued V and x as a wrong integer against the exact
NumPy product."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "accbpg_and_fw_amd", "csrc")
ROLLED = 1024                   # accbpg_debug_chol_variant: schedule 0 with the k-loop rolled over a runtime stage
BLOCK = 3 << 30                 # schedule 3

SMALL = [(768, 128), (768, 384), (768, 896), (768, 1536)]      # segments of 1, 2, 3, 4 (and 5) k-steps
CROSSING = [(1024, 1152), (1024, 2048)]                         # dual tiles; ranges that cross an entry boundary; tails behind trips
LONG = [(1024, 8192), (768, 81920)]                             # ten trips and more; hundreds of k-steps per segment
CHUNKED = [(768, 65536)]                                        # two column blocks: every segment through a slab
SHAPES = SMALL + CROSSING + LONG + CHUNKED

# one line per segment in the order a workgroup meets them: workgroup, range, dual tile?, k-steps
MAIN = r"""
#include "dopt_plan.hpp"
#include <stdio.h>
#include <stdlib.h>
using namespace accbpg;
int main(int argc, char** argv) {
    const int num_cu = atoi(argv[1]);
    for (int a = 2; a + 1 < argc; a += 2) {
        GramPlanIn in;
        in.m = atoll(argv[a]); in.n = atoll(argv[a + 1]); in.ldv = in.n;
        in.big = in.m >= 768; in.vec_ok = true; in.use_glds = true; in.num_cu = num_cu;
        const GramPlan p = plan_gram(in);
        if (!p.ok) return 1;
        printf("shape %lld %lld %d %lld %d\n", (long long)in.m, (long long)in.n, p.chunks, (long long)p.kiters, (int)p.has_duals);
        for (int w = 0; w < p.grid; ++w)
            for (int r = 0; r < GRAM_RMAX; ++r) {
                long long it = p.ranges[((size_t)w * GRAM_RMAX + r) * 2];
                const long long it1 = p.ranges[((size_t)w * GRAM_RMAX + r) * 2 + 1];
                while (it < it1) {
                    const long long e = it / p.kiters, off = it - e * p.kiters;
                    const bool dual = p.tiles[(size_t)e].d1 >= 0;
                    const GramSegK s = gram_segment_k(p.kiters, off, it1 - it, dual);
                    printf("seg %d %d %d %lld\n", w, r, (int)dual, (long long)(s.ke - s.kb));
                    it += s.ke - s.kb;
                }
            }
    }
    return 0;
}
"""


def _compiler():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    assert os.path.exists(rocm), "no host C++ compiler found"
    return rocm


@pytest.fixture(scope="module")
def acc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import accbpg_and_fw_amd as a
    return a


@pytest.fixture(scope="module")
def plans(acc, tmp_path_factory):
    """{(m, n): dict(chunks, kiters, duals, segs = [(workgroup, range, dual, k-steps)])} for this device's CU count"""
    d = tmp_path_factory.mktemp("gram_loop_plan")
    (d / "main.cpp").write_text(MAIN)
    exe = d / "plans"
    subprocess.check_call([_compiler(), "-std=c++17", "-O1", "-I", HEADER_DIR, str(d / "main.cpp"), "-o", str(exe)])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    args = [str(v) for s in SHAPES for v in s]
    out, cur = {}, None
    for line in subprocess.check_output([str(exe), str(cus)] + args, text=True).splitlines():
        f = line.split()
        if f[0] == "shape":
            cur = out.setdefault((int(f[1]), int(f[2])), dict(chunks=int(f[3]), kiters=int(f[4]), duals=int(f[5]), segs=[]))
        else:
            cur["segs"].append(tuple(int(v) for v in f[1:]))
    return out


def _plain_lengths(plan):
    return {L for (_, _, dual, L) in plan["segs"] if not dual}


def _second_starts(plan):
    """plain segments that start a pipeline behind another segment of the same workgroup: (same range, other range)"""
    same = other = 0
    seen = {}
    for w, r, dual, _ in plan["segs"]:
        if w in seen and not dual:
            if seen[w] == r:
                same += 1
            else:
                other += 1
        seen[w] = r
    return same, other


def test_shapes_reach_the_control_flow_they_are_there_for(plans):
    small = set().union(*[_plain_lengths(plans[s]) for s in SMALL])
    assert {1, 2, 3, 4} <= small and {L % 3 for L in small} == {0, 1, 2}, small
    # no trip at all (L <= 4), and one trip with a tail of 2, 3 and 4 steps (L = 5, 6, 7), two trips (L = 8, 9)
    cross = set().union(*[_plain_lengths(plans[s]) for s in CROSSING])
    assert {5, 6, 7, 8, 9} <= cross, cross
    assert all(plans[s]["duals"] for s in CROSSING) and any(dual for s in CROSSING for (_, _, dual, _) in plans[s]["segs"])
    same, other = _second_starts(plans[(1024, 2048)])
    assert same > 0, "no range of (1024, 2048) crosses an entry boundary"
    same, other = _second_starts(plans[(768, 896)])
    assert other > 0, "no workgroup of (768, 896) owns two ranges"
    assert max(_plain_lengths(plans[(1024, 8192)])) >= 32, _plain_lengths(plans[(1024, 8192)])
    # (the longest rows one column block takes with 11 tiles: n is no multiple of 32768)
    assert plans[(768, 81920)]["chunks"] == 1 and max(_plain_lengths(plans[(768, 81920)])) >= 200, _plain_lengths(plans[(768, 81920)])
    # (two column blocks of 32768 columns are the fewest a handle is cut into)
    assert plans[CHUNKED[0]]["chunks"] == 2 and plans[CHUNKED[0]]["kiters"] == 2048


def _handle_gram(f, x, bits):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    assert lib.accbpg_debug_chol_variant(f._h, bits) == 0
    G = torch.full((f.m, f.m), float("nan"), dtype=torch.float64, device="cuda")
    f.gram_into(x, G)
    torch.cuda.synchronize()
    return torch.tril(G)


def _timing_codes_run(f, x):
    """codes 28 (rolled) and 30 (constant stage) of accbpg_debug_gram_variant launch the two loops"""
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.functions import _ptr
    lib = _lib.load()
    ms = C.c_double(-1.0)
    for code in (28, 30):
        _lib.check(lib.accbpg_debug_gram_variant(f._h, _ptr(x), code, 1, C.byref(ms)), "accbpg_debug_gram_variant %d" % code)
        assert ms.value > 0.0, code


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_gram_matrix_has_the_same_bits_and_the_exact_integers(acc, plans, shape):
    """Integer-valued V (|v| <= 3) and x (1..4): every partial sum is an integer below 2^53, so the Gram matrix is exact
    whatever the order, and a misplaced fragment, stage or k-step is a wrong integer."""
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n = shape
    assert shape in plans
    gen = torch.Generator(device="cuda").manual_seed(11 * m + n)
    V = torch.randint(-3, 4, (m, n), device="cuda", generator=gen).to(torch.float64)
    x = torch.randint(1, 5, (n,), device="cuda", generator=gen).to(torch.float64)
    Vh, xh = V.cpu().numpy(), x.cpu().numpy()
    assert np.abs(Vh).max() * np.abs(Vh).max() * xh.max() * n < 2.0 ** 53
    exact = np.tril((Vh * xh) @ Vh.T)                           # float64 holds every partial sum of it exactly
    f = acc.DOptimalObj(V, _shard=(m >= n))                     # (the form that takes n <= m: only its Gram matrix is formed)
    try:
        new = _handle_gram(f, x, 0)
        rolled = _handle_gram(f, x, ROLLED)
        block = _handle_gram(f, x, BLOCK)
        if shape not in CHUNKED:                                # (the timing entry knows one column block only)
            _timing_codes_run(f, x)
        again = _handle_gram(f, x, 0)
    finally:
        lib.accbpg_debug_chol_variant(f._h, 0)
    assert np.array_equal(new.cpu().numpy(), exact)
    assert torch.equal(rolled, new) and torch.equal(block, new) and torch.equal(again, new)


FG_SHAPES = [s for s in SHAPES if s[1] > s[0]]                  # (n <= m: the Gram matrix is singular)


@pytest.mark.parametrize("shape", FG_SHAPES, ids=["%dx%d" % s for s in FG_SHAPES])
def test_value_and_gradient_have_the_same_bits(acc, shape):
    from accbpg_and_fw_amd import _lib
    lib = _lib.load()
    m, n = shape
    gen = torch.Generator(device="cuda").manual_seed(m + n)
    V = torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen)
    x = torch.rand(n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    x /= x.sum()
    f = acc.DOptimalObj(V)
    res = {}
    try:
        for bits in (0, ROLLED, BLOCK):
            assert lib.accbpg_debug_chol_variant(f._h, bits) == 0
            res[bits] = f.func_grad(x, 2)
            G = _handle_gram(f, x, bits)
            res[bits] = res[bits] + (G,)
    finally:
        lib.accbpg_debug_chol_variant(f._h, 0)
    f0, g0, G0 = res[0]
    assert np.isfinite(f0) and bool(torch.isfinite(g0).all())
    for bits in (ROLLED, BLOCK):
        fv, g, G = res[bits]
        assert fv == f0, bits
        assert torch.equal(g, g0), bits
        assert torch.equal(G, G0), bits


def test_lockstep_batch_with_an_inactive_instance(acc):
    """gram_streamk_glds_batch_kernel runs the same body with the production schedule.  (256, 384): m = 256 is the
    smallest row count at which a batch takes the 256 x 128 tile and with it the direct-to-LDS kernel, n = 384 the
    smallest multiple of 128 above m (the Gram matrix has to be positive definite for a value).  Each active instance's
    value and gradient are those of the instance evaluated alone under the rolled loop and under the block schedule; the
    inactive instance's row is left as it was."""
    from accbpg_and_fw_amd import _lib
    from accbpg_and_fw_amd.batched import DOptimalBatch
    lib = _lib.load()
    m, n, K = 256, 384, 3
    gen = torch.Generator(device="cuda").manual_seed(5)
    Vs = [torch.randn(m, n, dtype=torch.float64, device="cuda", generator=gen) for _ in range(K)]
    X = torch.rand(K, n, dtype=torch.float64, device="cuda", generator=gen) + 0.05
    X /= X.sum(1, keepdim=True)
    batch = DOptimalBatch(Vs)
    assert batch.fused
    active = [True, False, True]
    out = torch.full((K, n), -7.0, dtype=torch.float64, device="cuda")
    f, G = batch.func_grad(X, 2, active=active, out=out)
    torch.cuda.synchronize()
    assert np.isnan(f[1]) and bool((G[1] == -7.0).all())
    for i in (0, 2):
        inst = batch.instance(i)
        try:
            for bits in (ROLLED, BLOCK, 0):
                assert lib.accbpg_debug_chol_variant(inst._h, bits) == 0
                fi, gi = inst.func_grad(X[i], 2)
                assert f[i] == fi, (i, bits)
                assert torch.equal(G[i], gi), (i, bits)
        finally:
            lib.accbpg_debug_chol_variant(inst._h, 0)
