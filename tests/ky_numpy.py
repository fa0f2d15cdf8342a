"""NumPy restatement of the device Kumar-Yildirim start (csrc/kyinit_kernels.hip), written from its prose:
what accbpg_dopt_kyinit must return, bit for bit, given the same pass over V.

The arithmetic.  Every dot <Q[:,j], s> and every sum of squares over m entries is summed by one workgroup of 256 threads:
thread t folds the terms t, t + 256, ... in that order into an accumulator started at +0.0, then the block stage of the
fixed tree (tests/reduce_numpy.py: wave shuffles, then the four waves in wave order) -- a streaming reduction of ONE
block without a final stage, whatever m is.  Each term is one rounded product.  The deflation subtracts the rounded
products c_j * Q[:,j] in the order j = 0, 1, ..., exactly the reference's `q = q - Rij * Q[:,j]`, with every c_j taken
from the un-deflated vector.  The norm is the square root of the tree sum of q*q, and Q[:,i] = q / norm is a true division.
argmax / argmin are np.argmax / np.argmin (first index on ties, NaN kept).

The pass over V is a callable: plain `q @ V` on the CPU; on the GPU the device's own accbpg_dopt_vt_times, so that the
replay sees the bits the device's arg-extremum saw.
"""
import numpy as np

from reduce_numpy import THREADS, _add, _block_stage, _fold_rows


def tree_sums(terms):
    """terms[..., m] -> [...]: each row summed in the device's order (one block of 256 threads, no final stage)"""
    terms = np.asarray(terms, dtype=np.float64)
    m = terms.shape[-1]
    k = -(-m // THREADS)
    padded = np.zeros(terms.shape[:-1] + (k * THREADS,))        # +0.0 padding cannot change a bit (reduce_numpy._tree)
    padded[..., :m] = terms
    rows = np.moveaxis(padded.reshape(terms.shape[:-1] + (k, THREADS)), -2, 0)      # [k, ..., 256]
    with np.errstate(invalid="ignore", over="ignore"):
        return _block_stage(_fold_rows(rows, _add, 0.0), _add)


def deflate(QT, s):
    """s - sum_j <Q[:,j], s> Q[:,j] over the rows QT[j] = Q[:,j]: coefficients from the un-deflated s by the tree,
    subtracted in the order of j with a rounded product each"""
    c = tree_sums(QT * s) if len(QT) else np.zeros(0)
    q = np.copy(s)
    for j in range(len(QT)):
        q = q - c[j] * QT[j]
    return q


def normalize(q):
    with np.errstate(invalid="ignore", divide="ignore"):
        return q / np.sqrt(tree_sums(q * q))


def x0_from_picked(picked, n):
    """accbpg/applications.py:91-94"""
    x0 = np.zeros(n)
    x0[picked] = np.ones(len(picked)) / len(picked)
    x0 /= x0.sum()
    return x0


def kyinit(V, B, vt_times=None, steps=None):
    """The device's Kumar-Yildirim start for the directions B[i].  vt_times(q) -> q^T V as a NumPy vector (default q @ V).
    Returns picked (2m indices, [2i] = kmax, [2i+1] = kmin), Q (m x m, column j = direction j) and x0.
    steps: optional list that receives (q, w) of every step (the deflated direction and the pass over V it was given)."""
    V = np.asarray(V, dtype=np.float64)
    m, n = V.shape
    if vt_times is None:
        def vt_times(q):
            return q @ V
    QT = np.zeros((m, m))                   # row j = Q[:, j]
    picked = np.empty(2 * m, dtype=np.int64)
    for i in range(m):
        b = np.asarray(B[i], dtype=np.float64)
        q = deflate(QT[:i], b)
        w = np.asarray(vt_times(q))
        kmax = int(np.argmax(w))
        kmin = int(np.argmin(w))
        picked[2 * i], picked[2 * i + 1] = kmax, kmin
        if steps is not None:
            steps.append((q, w))
        v = V[:, kmin] - V[:, kmax]
        QT[i] = normalize(deflate(QT[:i], v))
    return picked, np.ascontiguousarray(QT.T), x0_from_picked(picked, n)


def draw_directions(m):
    """m calls of np.random.rand(m) in step order (accbpg/applications.py:74)"""
    return np.stack([np.random.rand(m) for _ in range(m)])


def smallest_gap(V, vt_times=None):
    """The oracle's recurrences (np.dot coefficients) on the legacy generator as it stands, with the smallest relative
    top-two gap over all 2m arg-extremum decisions: min over steps of (w_(1) - w_(2)) / max|w| at either end.  Returns
    (gap, x0); the generator ends where D_opt_KYinit leaves it.  vt_times(q) -> q^T V (default np.dot(q, V))."""
    m, n = V.shape
    if vt_times is None:
        def vt_times(q):
            return np.dot(q, V)
    Q = np.zeros((m, m))
    picked = []
    gap = np.inf
    for i in range(m):
        b = np.random.rand(m)
        q = np.copy(b)
        for j in range(i):
            q = q - np.dot(Q[:, j], b) * Q[:, j]
        w = np.asarray(vt_times(q))
        srt = np.sort(w)
        scale = np.max(np.abs(w))
        gap = min(gap, (srt[-1] - srt[-2]) / scale, (srt[1] - srt[0]) / scale)
        kmax, kmin = np.argmax(w), np.argmin(w)
        picked += [kmax, kmin]
        v = V[:, kmin] - V[:, kmax]
        q = np.copy(v)
        for j in range(i):
            q = q - np.dot(Q[:, j], v) * Q[:, j]
        Q[:, i] = q / np.linalg.norm(q)
    return gap, x0_from_picked(picked, n)
