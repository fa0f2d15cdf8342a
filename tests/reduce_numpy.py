"""NumPy emulator of the fixed reduction tree of the length-n kernels (csrc/reduce.hpp), written from
their prose: what the device must return for a sum or a minimum of per-entry float64 terms, bit for bit.

The tree.  A streaming reduction over n entries runs nb = min(max(ceil(n / 1024), 1), max_blocks) blocks of 256
threads.  Thread t of block b owns the entries b*256 + t + k*nb*256, k = 0, 1, ..., and folds them in that order into
an accumulator started at +0.0 (+inf for a minimum).  A block stage then reduces the 256 accumulators: inside each
wavefront of 64 lanes the pairwise tree v[l] = v[l] op v[l + off] for off = 32, 16, ..., 1 (only the pairs with
l < off reach lane 0), then the four wavefronts folded in wave order starting from wave 0's value.  That gives one
record per block.  A final stage of one block of 256 threads folds the records: thread t takes the records t, t + 256,
... in that order into an accumulator started at +0.0 (+inf), and the same block stage follows.  The kernels of
inexact_kernels.hip skip the final stage when nb == 1 (the block writes the result itself); `block_total` of the
Shannon simplex scale pass is the final stage of a sum.

The minimum is min_nan(a, b) = b if (b < a or b != b) else a at exactly the positions of the additions: it keeps a
NaN, as np.min does.

Caps (max_blocks): 1024 for vec_kernels.hip and inexact_kernels.hip, 512 for shannon_kernels.hip and
quartic_kernels.hip; accbpg_vec_argminmax stops at 128 blocks (its own merge, not emulated here: an arg-extremum is
exact in any order).
"""
import numpy as np

THREADS = 256                 # threads of a block of the streaming reductions
WAVE = 64                     # lanes of a wavefront
WAVES = THREADS // WAVE
PER_THREAD = 4                # entries per thread that the block-count rule aims at
PER_BLOCK = THREADS * PER_THREAD
CAP_VEC = 1024                # vec_kernels.hip, inexact_kernels.hip
CAP_WIDE = 512                # shannon_kernels.hip, quartic_kernels.hip (8-slot records)
CAP_ARG = 128                 # accbpg_vec_argminmax
RAGGED = 3 * 2 ** 20 + PER_BLOCK + 3      # many trips at either cap, the last one ragged (1027 entries of 131072+)
EPS = float(np.finfo(np.float64).eps)


def draw(n, seed):
    """the standard-normal test vector `seed` of length n (the CPU and the GPU tests draw the same data)"""
    return np.random.RandomState(7919 * seed + n % 1000003).randn(n)


def red_blocks(n, max_blocks):
    return min(max(-(-int(n) // PER_BLOCK), 1), int(max_blocks))


def edge_sizes(cap):
    """The sizes at which the tree of a kernel with this block cap changes shape, from the constants:
    one lane / one wave / one block's threads (+-1), nb 1 -> 2, the final stage's threads taking a second record,
    the cap exactly and one entry past it (the first two-trip size), and a multi-trip ragged size."""
    sizes = [1, WAVE - 1, WAVE, WAVE + 1, THREADS - 1, THREADS, THREADS + 1,
             PER_BLOCK - 1, PER_BLOCK, PER_BLOCK + 1,
             THREADS * PER_BLOCK, THREADS * PER_BLOCK + 1,
             cap * PER_BLOCK, cap * PER_BLOCK + 1, RAGGED]
    return sorted(set(sizes))


def planted_positions(n, cap):
    """Where one outlier is planted in otherwise constant data: the ends of a wave, a block's threads and a block's
    entries, the last entry of the first trip and the first of the second, and the tail."""
    nb = red_blocks(n, cap)
    want = [0, THREADS - 1, THREADS, PER_BLOCK - 1, PER_BLOCK, nb * THREADS - 1, nb * THREADS, n - THREADS - 1, n - 2,
            n - 1]
    return sorted(set(p for p in want if 0 <= p < n))


def trips(n, max_blocks):
    return -(-int(n) // (red_blocks(n, max_blocks) * THREADS))


def tree_depth(n, max_blocks, single_block_final=True):
    """The largest number of additions on a leaf-to-root path: the trips of a thread, 6 shuffle levels and 3 wave
    additions per stage, and ceil(nb / 256) record additions of the final stage."""
    nb = red_blocks(n, max_blocks)
    depth = trips(n, max_blocks) + 6 + (WAVES - 1)
    if nb > 1 or single_block_final:
        depth += -(-nb // THREADS) + 6 + (WAVES - 1)
    return depth


def _add(a, b):
    return a + b


def min_nan(a, b):
    return np.where((b < a) | (b != b), b, a)


def _block_stage(acc, op):
    """acc[..., 256] thread accumulators -> [...] block results"""
    v = acc.reshape(acc.shape[:-1] + (WAVES, WAVE))
    off = WAVE // 2
    while off > 0:
        v = op(v[..., :off], v[..., off:2 * off])
        off //= 2
    v = v[..., 0]
    a = v[..., 0]
    for w in range(1, WAVES):
        a = op(a, v[..., w])
    return a


def _fold_rows(rows, op, start):
    """rows[k, ...] folded over k in order into an accumulator started at `start`"""
    acc = np.full(rows.shape[1:], start, dtype=np.float64)
    for k in range(rows.shape[0]):
        acc = op(acc, rows[k])
    return acc


def _tree(values, max_blocks, op, start, single_block_final):
    values = np.ascontiguousarray(values, dtype=np.float64).ravel()
    n = values.size
    assert n >= 1
    nb = red_blocks(n, max_blocks)
    stride = nb * THREADS
    k = -(-n // stride)
    # Missing entries are padded with the start value.  For a sum that is +0.0: an accumulator started at +0.0 never
    # becomes -0.0 under round-to-nearest (+0.0 + -0.0 = +0.0, x + -x = +0.0), and s + 0.0 has the bits of s for every
    # other s, so the padding cannot change a bit.  For a minimum it is +inf, which min_nan never takes over a value.
    padded = np.full(k * stride, start, dtype=np.float64)
    padded[:n] = values
    with np.errstate(invalid="ignore", over="ignore"):
        acc = _fold_rows(padded.reshape(k, nb, THREADS), op, start)          # [nb, 256]
        rec = _block_stage(acc, op)                                          # [nb]
        if nb == 1 and not single_block_final:
            return np.float64(rec[0])
        r = -(-nb // THREADS)
        recs = np.full(r * THREADS, start, dtype=np.float64)
        recs[:nb] = rec
        fin = _fold_rows(recs.reshape(r, THREADS), op, start)                # [256]
        return np.float64(_block_stage(fin, op))


def tree_sum(terms, max_blocks, single_block_final=True):
    """The float64 the device returns for the sum of `terms` (per-entry float64 terms in entry order).
    single_block_final=False: the inexact kernels, whose single block writes the result without a final stage."""
    return _tree(terms, max_blocks, _add, 0.0, single_block_final)


def tree_min(values, max_blocks, single_block_final=True):
    """The float64 the device returns for the NaN-keeping minimum of `values`."""
    return _tree(values, max_blocks, min_nan, np.inf, single_block_final)
