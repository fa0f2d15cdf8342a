"""The emulator of the fixed reduction tree (tests/reduce_numpy.py) checked on the host, no GPU: its sizes hit the
shapes they are meant to hit, integer data sums exactly, random data stays within tree_depth * eps * sum|terms| of the
correctly rounded sum (math.fsum), and the minimum is np.min, NaN included.  The GPU tests (test_gpu_reduce.py) hold
the device bit-equal to this emulator and inherit the evidence that emulator and reference meet the bound on the
inputs used there (the same generator, `terms_for`)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_numpy as T  # noqa: E402

CAPS = [T.CAP_WIDE, T.CAP_VEC]
CASES = [(cap, n) for cap in CAPS for n in T.edge_sizes(cap)]


def terms_for(n, seed=0):
    """random terms of mixed sign and magnitude (products of normals), as the GPU tests draw them"""
    return T.draw(n, 2 * seed) * T.draw(n, 2 * seed + 1)


@pytest.mark.parametrize("cap", CAPS)
def test_sizes_hit_every_shape_of_the_tree(cap):
    sizes = T.edge_sizes(cap)
    nbs = {n: T.red_blocks(n, cap) for n in sizes}
    assert 1 in nbs.values() and 2 in nbs.values()                            # nb == 1 and nb == 2
    assert nbs[T.PER_BLOCK] == 1 and nbs[T.PER_BLOCK + 1] == 2
    assert T.THREADS in nbs.values() and T.THREADS + 1 in nbs.values()        # 256 and 257 records in the final stage
    at_cap = [n for n in sizes if nbs[n] == cap and T.trips(n, cap) == T.PER_THREAD and n % (cap * T.THREADS) == 0]
    assert at_cap == [cap * T.PER_BLOCK]                                      # the cap exactly: four full trips
    past = cap * T.PER_BLOCK + 1
    assert past in sizes and nbs[past] == cap and T.trips(past, cap) == T.PER_THREAD + 1      # one entry past it
    assert nbs[T.RAGGED] == cap and T.trips(T.RAGGED, cap) > 2 * T.PER_THREAD                 # many trips,
    assert T.RAGGED % (cap * T.THREADS) != 0 and T.RAGGED % T.THREADS != 0                    # the last one ragged
    assert cap > T.THREADS                      # at the cap every final-stage thread holds two or more records
    for n in sizes:
        assert T.planted_positions(n, cap)[-1] == n - 1
    assert max(sizes) < 3.2e6


def test_block_count_and_depth():
    assert T.red_blocks(0, 8) == 1 and T.red_blocks(1, 8) == 1 and T.red_blocks(1024, 8) == 1
    assert T.red_blocks(1025, 8) == 2 and T.red_blocks(10 ** 9, 8) == 8
    # one trip, one block stage (6 shuffles + 3 waves), a final stage with one record per thread
    assert T.tree_depth(1, T.CAP_VEC) == 1 + 9 + 1 + 9
    assert T.tree_depth(1, T.CAP_VEC, single_block_final=False) == 1 + 9
    assert T.tree_depth(1025, T.CAP_VEC, single_block_final=False) == 3 + 9 + 1 + 9
    assert T.tree_depth(T.CAP_VEC * T.PER_BLOCK + 1, T.CAP_VEC) == 5 + 9 + 4 + 9
    assert T.tree_depth(T.RAGGED, T.CAP_WIDE) == 25 + 9 + 2 + 9


@pytest.mark.parametrize("cap,n", CASES)
def test_integer_terms_sum_exactly(cap, n):
    rng = np.random.RandomState(n)
    terms = rng.randint(-1000, 1001, size=n).astype(np.float64)
    for final in (True, False):
        assert T.tree_sum(terms, cap, final) == float(int(terms.sum()))
    # one outlier in constant data, at every planted position
    for p in T.planted_positions(n, cap):
        v = np.full(n, 3.0)
        v[p] += 1000.0
        assert T.tree_sum(v, cap) == 3.0 * n + 1000.0


@pytest.mark.parametrize("cap,n", CASES)
def test_random_terms_within_the_depth_bound(cap, n):
    terms = terms_for(n)
    got = T.tree_sum(terms, cap)
    ref = math.fsum(terms)
    bound = T.tree_depth(n, cap) * T.EPS * math.fsum(np.abs(terms))
    print("cap %d n %d depth %d err %.3e bound %.3e" % (cap, n, T.tree_depth(n, cap), abs(got - ref), bound))
    assert abs(got - ref) <= bound
    # the skipped final stage of a single block changes no bit (0.0 + record, then additions of +0.0)
    assert T.tree_sum(terms, cap, single_block_final=False) == got


@pytest.mark.parametrize("cap,n", CASES)
def test_minimum_is_np_min_and_keeps_a_nan(cap, n):
    vals = terms_for(n, seed=1)
    assert T.tree_min(vals, cap) == vals.min()
    assert T.tree_min(vals, cap, single_block_final=False) == vals.min()
    for p in T.planted_positions(n, cap):
        v = np.full(n, 2.0)
        v[p] = -7.0
        assert T.tree_min(v, cap) == -7.0 == np.min(v)
        v[p] = np.nan
        assert np.isnan(T.tree_min(v, cap)) and np.isnan(np.min(v))
        assert np.isnan(T.tree_min(v, cap, single_block_final=False))
    assert T.tree_min(np.full(n, np.inf), cap) == np.inf


def test_the_tree_is_the_documented_one_on_a_hand_case():
    """n = 130 at one block: thread t holds entry t; wave 0 is the pairwise tree over 64 lanes, wave 1 likewise, wave
    2 holds two entries; waves folded in order; the final stage adds 0.0 + record and zeros."""
    rng = np.random.RandomState(5)
    t = rng.randn(130) * 10.0 ** rng.randint(-8, 8, size=130)

    def wave(v):
        v = list(v) + [0.0] * (64 - len(v))
        off = 32
        while off:
            for lane in range(off):
                v[lane] = v[lane] + v[lane + off]
            off //= 2
        return v[0]

    expect = ((wave(t[:64]) + wave(t[64:128])) + wave(t[128:])) + 0.0
    assert T.tree_sum(t, T.CAP_VEC) == expect
    # two blocks (n = 1025): block b, thread t holds entries b*256 + t + k*512
    t = rng.randn(1025) * 10.0 ** rng.randint(-8, 8, size=1025)
    recs = []
    for b in range(2):
        acc = [0.0] * 256
        for k in range(3):
            for th in range(256):
                i = b * 256 + th + k * 512
                if i < 1025:
                    acc[th] = acc[th] + t[i]
        recs.append(((wave(acc[:64]) + wave(acc[64:128])) + wave(acc[128:192])) + wave(acc[192:]))
    expect = ((wave([0.0 + recs[0], 0.0 + recs[1]]) + 0.0) + 0.0) + 0.0
    assert T.tree_sum(t, T.CAP_VEC) == expect
