"""Host-side helpers of accbpg/utils.py: the LIBSVM / svmlight text reader (:22-95, returns
(scipy.sparse.csr_matrix, labels); the matrix goes to the GPU when an objective is built on it) and the random
points and inexactness levels of the simplex experiments (:252-295), which draw from NumPy's legacy global
generator exactly as the reference does.

The file is tokenised once and the index / value columns are converted, validated and assembled into CSR
with array operations (no per-entry Python work), which is what the datasets this package is pointed at
(hundreds of thousands of entries) want."""
from __future__ import annotations

import bz2
import gzip
import os.path

import numpy as np
import scipy.sparse as sparse

_OPENERS = {".gz": gzip.open, ".bz2": bz2.open}


def _read_text(filename):
    opener = _OPENERS.get(os.path.splitext(filename)[1], open)
    with opener(filename, "rt") as fh:
        return fh.read()


def _first_violation(ids, row_of, zero_based):
    """Position and kind of the first malformed entry in file order, or None."""
    bad_index = ids < 0
    if not zero_based:                                   # (the string "auto" counts as true here)
        bad_index |= ids == 0
    unsorted = np.zeros(ids.shape, dtype=bool)
    unsorted[1:] = (row_of[1:] == row_of[:-1]) & (ids[1:] <= ids[:-1])
    where = np.flatnonzero(bad_index | unsorted)
    if where.size == 0:
        return None
    at = int(where[0])
    return at, ("index" if bad_index[at] else "order")


def load_libsvm_file(filename, dtype=np.float64, n_features=None, zero_based="auto"):
    """Each record is ``label idx:value idx:value ...``; '#' starts a comment; blank records are skipped.
    Indices must be increasing within a record.  zero_based="auto" treats the file as one-based when its
    smallest index is positive; n_features grows (with a printed warning) when the data need more columns."""
    records = [body.split() for body in (ln.split("#", 1)[0] for ln in _read_text(filename).splitlines())]
    records = [rec for rec in records if rec]
    labels = np.array([float(rec[0]) for rec in records])
    per_row = np.fromiter((len(rec) - 1 for rec in records), dtype=np.int64, count=len(records))
    pairs = [tok.split(":", 1) for rec in records for tok in rec[1:]]
    ids = np.array([p[0] for p in pairs]).astype(np.int64) if pairs else np.zeros(0, dtype=np.int64)
    row_of = np.repeat(np.arange(len(records)), per_row)

    problem = _first_violation(ids, row_of, zero_based)
    if problem is not None:
        at, kind = problem
        if kind == "index":
            raise ValueError("Invalid index {0:d} in LibSVM data file.".format(int(ids[at])))
        raise ValueError("Feature indices in LibSVM data file"
                         "should be sorted and unique.")
    vals = np.array([dtype(p[1]) for p in pairs])

    one_based = (zero_based is False) or (zero_based == "auto" and ids.min() > 0)
    if one_based:
        ids = ids - 1
    width = int(ids.max()) + 1
    if n_features is not None and n_features < width:
        print("Warning: n_features increased to match data.")
    if n_features is None or n_features < width:
        n_features = width
    row_ptr = np.concatenate(([0], np.cumsum(per_row)))
    X = sparse.csr_matrix((vals, ids, row_ptr), (len(records), n_features))
    X.sort_indices()
    return X, labels


def random_point_on_simplex(n, radius=1, center=False):
    """The centre ones(n)/n, or the gaps between n-1 sorted draws of uniform(0.01, radius) padded with 0 and radius
    (accbpg/utils.py:252-268): one np.random.uniform(size=n-1) call, none for the centre."""
    if center:
        return np.ones(n) / n
    cuts = np.random.uniform(low=0.01, high=radius, size=(n - 1,))
    cuts.sort()
    return np.diff(np.concatenate([[0], cuts, [radius]]))


def edge_point_on_simplex(edge_index, n, radius=1, tol=1e-5):
    """tol everywhere and radius - tol*(n-1) at edge_index (accbpg/utils.py:271-275)."""
    x = np.zeros(n) + tol
    x[edge_index] = radius - tol * (n - 1)
    return x


def get_random_float(var=1):
    """var * np.random.random_sample(), or the integer 0 without a draw when var == 0 (accbpg/utils.py:278-285)."""
    if var == 0:
        return 0
    assert var > 0, 'The range must be positive.'
    val = var * np.random.random_sample()
    assert val > 0
    return val


def get_random_vector(size, range=1):
    """range * np.random.random_sample(size), or zeros without a draw when range == 0 (accbpg/utils.py:288-295)."""
    if range == 0:
        return np.zeros(size)
    assert range > 0, 'The range must be positive.'
    vec = range * np.random.random_sample(size=size)
    assert vec.min() > 0
    return vec


def generate_dataset_for_svm(m, n):
    """m rows of 100*N(0,1) entries from a fresh np.random.default_rng() (one standard_normal(n) call per row), label
    +1 where fewer than 0.53*n entries of the row are positive and -1 otherwise (accbpg/utils.py:161-192).  Returns
    (data, labels); the generator is unseeded, as in the reference."""
    data = []
    labels = []
    rng = np.random.default_rng()
    variance = 100
    for _ in range(m):
        row = rng.standard_normal(n) * variance
        labels.append(1 if (row > 0).sum() < n * 0.53 else -1)
        data.append(row)
    return np.array(data), np.array(labels)


def random_point_in_l2_ball(center, radius, spread_btm=0.1, spread_up=0.99, pos_dir=False):
    """center + rho*d with d = np.random.randn(n) normalised (made entrywise nonnegative when pos_dir) and rho =
    np.random.uniform(radius*spread_btm, radius*spread_up), in this order of draws from the global generator
    (accbpg/utils.py:195-212)."""
    ndim = len(center)
    direction = np.random.randn(ndim)
    direction /= np.linalg.norm(direction)
    if pos_dir:
        direction = np.sign(direction) * direction
    rho = np.random.uniform(radius * spread_btm, radius * spread_up)
    point = center + rho * direction
    assert np.linalg.norm(point - center) - radius <= 1e-15
    return point
