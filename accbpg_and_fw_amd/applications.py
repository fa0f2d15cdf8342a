"""Problem factories (accbpg/applications.py): D-optimal design, Poisson and KL regression (on the orthant and on the
simplex), symmetric NMF, the soft-margin SVM on an l2 ball, and l1-regularised logistic regression in a box."""
from __future__ import annotations

import numpy as np

from .functions import (BurgEntropyL1, BurgEntropyL2, BurgEntropySimplex, DOptimalObj, FrobeniusSymLoss,
                        KLdivRegression, L2L1Linf, LogisticRegression, PoissonRegression, PolyDiv, ShannonEntropyL1,
                        SquaredL2Norm, SumOf2nd4thPowers, SumOf2nd4thPowersPositiveOrthant, SVM_fun, vec_argminmax)
from .utils import (edge_point_on_simplex, generate_dataset_for_svm, load_libsvm_file, random_point_in_l2_ball,
                    random_point_on_simplex)


def D_opt_libsvm(filename):
    """D-optimal design instance from a LIBSVM data file (accbpg/applications.py:17-33): the data
    matrix, transposed when it has more rows than columns, is the m x n design matrix."""
    X, y = load_libsvm_file(filename)
    if X.shape[0] > X.shape[1]:
        H = X.T.toarray('C')
    else:
        H = X.toarray('C')
    n = H.shape[1]
    f = DOptimalObj(H)
    h = BurgEntropySimplex()
    L = 1.0
    x0 = (1.0 / n) * np.ones(n)
    return f, h, L, x0


def D_opt_KYinit(V):
    """Sparse Kumar-Yildirim starting point (accbpg/applications.py:59-95).  ``V`` is the design
    matrix or a DOptimalObj over it.  The m passes over V (q^T V, argmax / argmin, two column reads)
    run on the GPU; the length-m Gram-Schmidt recurrences stay on the host in the reference's order
    (coefficients from the un-deflated vector, :75-78 and :86-89), with the same legacy-RNG draws
    (np.random.rand(m) per direction, :74)."""
    obj = V if isinstance(V, DOptimalObj) else None
    m, n = (obj.m, obj.n) if obj is not None else V.shape
    if n <= 2 * m:
        return (1.0 / n) * np.ones(n)
    if obj is None:
        obj = DOptimalObj(V)

    picked = []
    Q = np.zeros((m, m))
    for i in range(m):
        b = np.random.rand(m)
        q = np.copy(b)
        for j in range(i):
            q = q - np.dot(Q[:, j], b) * Q[:, j]
        kmin, kmax, _, _ = vec_argminmax(obj.vt_times(q))       # :79-81
        picked.append(kmax)
        picked.append(kmin)
        v = obj.column(kmin) - obj.column(kmax)                 # :84
        q = np.copy(v)
        for j in range(i):
            q = q - np.dot(Q[:, j], v) * Q[:, j]
        Q[:, i] = q / np.linalg.norm(q)

    x0 = np.zeros(n)
    x0[picked] = np.ones(len(picked)) / len(picked)
    x0 /= x0.sum()                                              # repeated indices: rescale to sum 1 (:93-94)
    return x0


def D_opt_KYinit_device(V, return_picked=False):
    """D_opt_KYinit with all m steps decided on the device (accbpg_dopt_kyinit): the Gram-Schmidt recurrences, the pass
    over V, the arg-extrema and the column reads are enqueued in one call and the host waits once.  ``V`` is the design
    matrix or a DOptimalObj over it.  The directions are drawn here, m calls of np.random.rand(m) in step order
    (accbpg/applications.py:74), so the legacy generator ends in the state the reference leaves it in; for n <= 2m the
    uniform point is returned without touching it (:67).  x0 is formed on the host as in :91-94.
    ``return_picked=True`` returns (x0, picked) with picked[2i] = kmax, picked[2i+1] = kmin of step i.

    The result equals D_opt_KYinit's for the same RNG state whenever no arg-max or arg-min decision lies within rounding
    of a tie: the device sums each Gram-Schmidt dot product in its own fixed order, not in np.dot's.  Such ties are
    not exotic -- q is orthogonal to every earlier v = V[:,kmin] - V[:,kmax], so the two members of every earlier pair
    have equal q^T V by construction, and when such a pair is the extreme any two summation orders may pick
    differently."""
    obj = V if isinstance(V, DOptimalObj) else None
    m, n = (obj.m, obj.n) if obj is not None else V.shape
    if n <= 2 * m:
        x0 = (1.0 / n) * np.ones(n)
        return (x0, np.zeros(0, dtype=np.int64)) if return_picked else x0
    if obj is None:
        obj = DOptimalObj(V)

    B = np.empty((m, m))
    for i in range(m):
        B[i] = np.random.rand(m)                                # :74
    picked = obj.kyinit_picks(B)

    x0 = np.zeros(n)
    x0[picked] = np.ones(len(picked)) / len(picked)             # fancy assignment, not accumulation (:92)
    x0 /= x0.sum()                                              # :93-94
    return (x0, picked) if return_picked else x0


def D_opt_KYinit_batch(batch, return_picked=False):
    """D_opt_KYinit_device for the K instances of a ``DOptimalBatch`` in lock-step (accbpg_dopt_batch_kyinit): every
    launch of a step covers all instances, and the host waits once for all K starts.  ``batch`` is a DOptimalBatch or a
    sequence of K matrices of one shape, from which one is built.  The directions are drawn here instance by instance,
    m calls of np.random.rand(m) each in step order, so the legacy generator ends exactly where the loop
    ``for i: D_opt_KYinit_device(batch.instance(i))`` leaves it; for n <= 2m the K x n uniform array is returned without
    touching the generator, without building a batch and without a GPU.  Returns the K x n array of starts (what
    D_opt_FW_batch and its variants take as x0), row i bit for bit ``D_opt_KYinit_device(batch.instance(i))``; with
    ``return_picked=True`` also the K x 2m indices, [i, 2s] = kmax, [i, 2s+1] = kmin of instance i's step s."""
    from .batched import DOptimalBatch
    if isinstance(batch, DOptimalBatch):
        K, m, n = batch.K, batch.m, batch.n
    else:
        K = len(batch)
        assert K > 0, "D_opt_KYinit_batch: no instances"
        m, n = batch[0].shape
        assert all(tuple(V.shape) == (m, n) for V in batch), "D_opt_KYinit_batch: instances must have one shape"
    if n <= 2 * m:
        X0 = (1.0 / n) * np.ones((K, n))
        return (X0, np.zeros((K, 0), dtype=np.int64)) if return_picked else X0
    if not isinstance(batch, DOptimalBatch):
        batch = DOptimalBatch(batch)

    B = np.empty((K, m, m))
    for i in range(K):
        for s in range(m):
            B[i, s] = np.random.rand(m)                         # :74
    picked = batch.kyinit_picks(B)

    X0 = np.empty((K, n))
    for i in range(K):
        x0 = np.zeros(n)
        x0[picked[i]] = np.ones(2 * m) / (2 * m)                # fancy assignment, not accumulation (:92)
        x0 /= x0.sum()                                          # :93-94
        X0[i] = x0
    return (X0, picked) if return_picked else X0


def D_opt_design(m, n, randseed=-1):
    """Random Gaussian instance: returns (f, h, L, x0) with f = DOptimalObj(H),
    h = BurgEntropySimplex(), L = 1, x0 = centre of the simplex.  As in the reference
    the legacy global NumPy generator is seeded only if randseed > 0
    (applications.py:47-49), so the same seed gives the same H on both sides."""
    if randseed > 0:
        np.random.seed(randseed)
    H = np.random.randn(m, n)
    f = DOptimalObj(H)
    h = BurgEntropySimplex()
    L = 1.0
    x0 = (1.0 / n) * np.ones(n)
    return f, h, L, x0


def _poisson_instance(m, n, noise, randseed, normalizeA):
    """(A, b) of the random Poisson linear inverse problem (accbpg/applications.py:114-123, 153-162):
    legacy global RNG drawn in the order A, x, noise; generated on the host like the reference's."""
    if randseed > 0:
        np.random.seed(randseed)
    A = np.random.rand(m, n)
    if normalizeA:
        A = A / A.sum(axis=0)
    x = np.random.rand(n) / n
    xavg = x.sum() / x.size
    x = np.maximum(x - xavg, 0) * 10
    b = np.dot(A, x) + noise * (np.random.rand(m) - 0.5)
    assert b.min() > 0, "need b > 0 for nonnegative regression."
    return A, b


def Poisson_regrL1(m, n, noise=0.01, lamda=0, randseed=-1, normalizeA=True):
    """minimize_{x >= 0} D_KL(b, Ax) + lamda*||x||_1  (accbpg/applications.py:98-133).
    Returns f, h, L = ||b||_1, x0 = (10/n)*ones."""
    A, b = _poisson_instance(m, n, noise, randseed, normalizeA)
    return PoissonRegression(A, b), BurgEntropyL1(lamda), b.sum(), (1.0 / n) * np.ones(n) * 10


def Poisson_regrL2(m, n, noise=0.01, lamda=0, randseed=-1, normalizeA=True):
    """minimize_{x >= 0} D_KL(b, Ax) + (lamda/2)*||x||_2^2  (accbpg/applications.py:136-172).
    Returns f, h, L = ||b||_1, x0 = (1/n)*ones."""
    A, b = _poisson_instance(m, n, noise, randseed, normalizeA)
    return PoissonRegression(A, b), BurgEntropyL2(lamda), b.sum(), (1.0 / n) * np.ones(n)


def KL_nonneg_regr(m, n, noise=0.01, lamdaL1=0, randseed=-1, normalizeA=True):
    """minimize_{x >= 0} D_KL(Ax, b) + lamdaL1*||x||_1  (accbpg/applications.py:175-206): legacy global RNG drawn
    in the order A, x, noise, on the host like the reference's.  Returns f = KLdivRegression, h = ShannonEntropyL1,
    L = max column sum of A, x0 = 0.5*ones."""
    if randseed > 0:
        np.random.seed(randseed)
    A = np.random.rand(m, n)
    if normalizeA:
        A = A / A.sum(axis=0)
    x = np.random.rand(n)
    b = np.dot(A, x) + noise * (np.random.rand(m) - 0.5)
    assert b.min() > 0, "need b > 0 for nonnegative regression."
    return KLdivRegression(A, b), ShannonEntropyL1(lamdaL1), max(A.sum(axis=0)), 0.5 * np.ones(n)


def _simplex_instance(m, n, noise, normalizeA, solution):
    """(A, b) with b = A solution + noise*rand(m) (accbpg/applications.py:212-217, 250-255): the legacy global RNG drawn
    in the order A, noise, on the host like the reference's."""
    A = np.random.rand(m, n)
    if normalizeA:
        A = A / A.sum(axis=0)
    b = np.dot(A, solution) + noise * (np.random.rand(m))
    assert b.min() > 0, "need b > 0 for nonnegative regression."
    return A, b


def Poisson_regr_simplex_acc(m, n, noise=0.01, normalizeA=True):
    """minimize_{x in simplex} D_KL(b, Ax) for the inexact-oracle accelerated methods (accbpg/applications.py:209-224).
    Draws x0, the solution, A and the noise in that order.  Returns f, [BurgEntropySimplex(eps=1e-7), SquaredL2Norm()],
    L = ||b||_1, x0 (a random point of the simplex)."""
    x0 = random_point_on_simplex(n, center=False)
    solution = random_point_on_simplex(n, center=False)
    A, b = _simplex_instance(m, n, noise, normalizeA, solution)
    f = PoissonRegression(A, b)
    L = np.abs(b).sum()
    h = BurgEntropySimplex(eps=1e-7)
    h_euklid = SquaredL2Norm()
    return f, [h, h_euklid], L, x0


def Poisson_regr_simplex(m, n, noise=0.01, normalizeA=True):
    """Four instances of minimize_{x in simplex} D_KL(b, Ax) that differ in where x0 and the solution lie
    (accbpg/applications.py:227-295).  Returns h = BurgEntropySimplex() and a dict placement -> (f, L = sum(b), solution,
    x0), generated in the reference's order: for each placement x0, solution, then A and the noise."""
    key1 = 'x0_center_sol_center'
    key2 = 'x0_edge_sol_edge'
    key3 = 'x0_edge_sol_center'
    key4 = 'x0_center_sol_edge'

    def generate_problem(solution_and_x0):
        solution, x0 = solution_and_x0
        A, b = _simplex_instance(m, n, noise, normalizeA, solution)
        return PoissonRegression(A, b), b.sum(), solution, x0

    def generate_sol_and_x0(place):
        if place == key1:
            x0 = random_point_on_simplex(n, center=True)
            solution = random_point_on_simplex(n)
        elif place == key2:
            x0 = edge_point_on_simplex(np.random.randint(n), n)
            solution = edge_point_on_simplex(np.random.randint(n), n)
        elif place == key3:
            x0 = edge_point_on_simplex(np.random.randint(n), n)
            solution = random_point_on_simplex(n, center=True)
        elif place == key4:
            x0 = random_point_on_simplex(n, center=True)
            solution = edge_point_on_simplex(np.random.randint(n), n)
        else:
            assert 0, 'Place had not been defined'
        return solution, x0

    points_positions = {key: generate_problem(generate_sol_and_x0(key)) for key in (key1, key2, key3, key4)}
    h = BurgEntropySimplex()
    return h, points_positions


def _symnmf_l2_instance(n, r, ball_center, radius=1.0, on_boundary=True):
    """(M, X0) of FrobeniusSymLossExL2Ball on the host: the legacy global RNG drawn in the reference's order
    (accbpg/applications.py:330-352), with its assertions."""
    rows = n
    X = np.random.randn(n, r)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    if on_boundary:
        X *= radius
    else:
        scales = np.random.uniform(0, 1, size=(n, 1)) ** (1 / r)
        X *= radius * scales
    X += ball_center

    assert np.all(X >= 0), "X must be non-negative"
    distances_l2_ball = np.linalg.norm(X - ball_center, axis=1)
    if on_boundary:
        assert np.all(np.abs(distances_l2_ball - radius) < 1e-6), "Some points are not on L2 ball boundary"
    else:
        assert np.all(distances_l2_ball <= radius + 1e-6), "Some points lie outside the L2 ball"

    approx_matrix = X.dot(X.T)
    assert np.allclose(approx_matrix, approx_matrix.T), "matrix must be symmetric"
    assert np.all(approx_matrix >= 0), "approx_matrix must be non-negative"
    assert approx_matrix.shape[0] == approx_matrix.shape[1], "approx_matrix must be square"

    X0 = np.ones((rows, r)) * radius + 1e-5 * radius
    assert np.all(X0 >= 0), "X0 must be non-negative"
    return approx_matrix, X0


def _symnmf_linf_instance(n, r, ball_center, radius=1.0, on_boundary=True):
    """(M, X0) of FrobeniusSymLossExLInfBall on the host (accbpg/applications.py:363-392), same RNG order and
    assertions."""
    X = np.random.randn(n, r)
    X /= np.max(np.abs(X))
    if on_boundary:
        X *= radius
    else:
        X *= radius * np.random.uniform(0, 1)
    X += ball_center

    assert np.all(X >= 0), "X must be non-negative"
    distances_linf_ball = np.max(np.abs(X - ball_center))
    if on_boundary:
        assert np.abs(distances_linf_ball - radius) <= 1e-6, "X is not on L∞ ball boundary"
    else:
        assert distances_linf_ball <= radius + 1e-6, "X is outside the L∞ ball"

    approx_matrix = X @ X.T
    assert np.allclose(approx_matrix, approx_matrix.T), "approx_matrix must be symmetric"
    assert np.all(approx_matrix >= 0), "approx_matrix must be non-negative"

    X0 = np.ones((n, r)) * radius + 1e-5 * radius
    assert np.all(X0 >= 0), "X0 must be non-negative"
    assert np.max(np.abs(X0 - ball_center)) < radius
    return approx_matrix, X0


def FrobeniusSymLossExL2Ball(n, r, ball_center, radius=1.0, on_boundary=True):
    """SymNMF instance M = X X^T with the rows of X on (or inside) an l2 ball (accbpg/applications.py:330-360).
    Returns f = FrobeniusSymLoss, h = SumOf2nd4thPowers(6, 2*||M||_2), L = 1, X0 and M (NumPy)."""
    approx_matrix, X0 = _symnmf_l2_instance(n, r, ball_center, radius, on_boundary)
    f = FrobeniusSymLoss(approx_matrix, X0)
    L = 1
    alpha = 6
    sigma = 2 * np.linalg.norm(approx_matrix, 2)
    h = SumOf2nd4thPowers(alpha, sigma)
    return f, h, L, X0, approx_matrix


def FrobeniusSymLossExLInfBall(n, r, ball_center, radius=1.0, on_boundary=True):
    """SymNMF instance M = X X^T with X on (or inside) an l-infinity ball (accbpg/applications.py:363-399).
    Returns f, h = SumOf2nd4thPowers(6, 2*||M||_2), L = 1, X0 and M (NumPy)."""
    approx_matrix, X0 = _symnmf_linf_instance(n, r, ball_center, radius, on_boundary)
    f = FrobeniusSymLoss(approx_matrix, X0)
    L = 1
    alpha = 6
    sigma = 2 * np.linalg.norm(approx_matrix, 2)
    h = SumOf2nd4thPowers(alpha, sigma)
    return f, h, L, X0, approx_matrix


def FrobeniusSymLossResMeasEx(M, r, noise=0.0):
    """SymNMF of a given symmetric M from X0 = rand(n, r) (accbpg/applications.py:402-415).  Returns f,
    [SumOf2nd4thPowersPositiveOrthant(6, 2*||M||_2), SquaredL2Norm()], L = 1, X0.  As in the reference, `noise`
    is not passed on."""
    X0 = np.random.rand(M.shape[0], r)
    assert np.all(X0 >= 0) >= 0, "X0 must be non-negative"
    f = FrobeniusSymLoss(M, X0)
    h = SumOf2nd4thPowersPositiveOrthant(6, 2 * np.linalg.norm(M, 2), upper_bound=None)
    h_euklid = SquaredL2Norm()
    L = 1
    return f, [h, h_euklid], L, X0


def _svm_ball_numbers(X, Y, lamda, center):
    """The host arithmetic of svm_digits_ds_divs_ball (accbpg/applications.py:317-325) -> (radius, DS_mean,
    DS_mean_quad, L, x0): the radius from the row norms of X without its last column, the reference's upper bound of
    L, and x0 drawn from the global NumPy generator (random_point_in_l2_ball)."""
    n = X.shape[1]
    radius = min(n ** -1 * lamda ** -1 * np.sum(np.linalg.norm(X[:, :-1], axis=1)), (2 / lamda) ** 0.5)
    if center is None:
        center = np.zeros(n)
    ds_mean = np.mean(np.linalg.norm(X, axis=1))
    ds_mean_quad = np.mean(np.linalg.norm(X, axis=1) ** 2)
    L = (ds_mean + min((2 * lamda) ** 0.5, ds_mean_quad)) * 0.08
    x0 = random_point_in_l2_ball(center, radius, pos_dir=False)
    return radius, ds_mean, ds_mean_quad, L, x0


def svm_digits_ds_divs_ball(center=None, lamda=0.5, real_ds=False):
    """Binary soft-margin SVM on an l2 ball (accbpg/applications.py:298-327): the two-class digits set of scikit-learn
    (real_ds, labels -1 / +1) or generate_dataset_for_svm(700, 2000).  Returns f, [PolyDiv, SquaredL2Norm], L, x0,
    radius with the reference's radius, L and x0 (one randn(n) and one uniform from the global generator)."""
    if real_ds:
        from sklearn.datasets import load_digits
        X, Y = load_digits(n_class=2, return_X_y=True, as_frame=True)
        Y = (Y > 0).astype(int) * 2 - 1
        X = X.to_numpy()
        Y = Y.to_numpy()
    else:
        X, Y = generate_dataset_for_svm(700, 2000)
    f = SVM_fun(lamda, X, Y)
    radius, _, _, L, x0 = _svm_ball_numbers(X, Y, lamda, center)
    poly_h, sqL2_h = PolyDiv(X, lamda=lamda, radius=radius), SquaredL2Norm()
    return f, [poly_h, sqL2_h], L, x0, radius


def Logistic_regr_L2L1Linf(m, n, lamda=None, B=1, randseed=-1, labels=None):
    """l1-regularised logistic regression in the box ||x||_inf <= B (accbpg/ex_LR_L2L1Linf.py:57-70):
        minimize_x  (1/m) * sum_i log(1 + exp(-b_i*(ai'*x))) + lamda*||x||_1   subject to ||x||_inf <= B.
    The draws are the example's, in its order, from the legacy global generator: A = randn(m, n), then
    b = sign(rand(m, 1)) -- all +1, kept so that a seeded script consumes the same stream.  ``labels`` (length m),
    when given, replaces b after the draws; ``lamda`` defaults to 1.0/m.  Returns f, h = L2L1Linf(lamda, B),
    L = 0.25, x0 = zeros(n)."""
    if randseed > 0:
        np.random.seed(randseed)
    A = np.random.randn(m, n)
    b = np.sign(np.random.rand(m, 1))
    if labels is not None:
        b = np.asarray(labels, dtype=np.float64)
        assert b.size == m, "Logistic Regression: len(b) != m"
    f = LogisticRegression(A, b.reshape(-1))
    h = L2L1Linf(lamda=1.0 / m if lamda is None else lamda, B=B)
    L = 0.25
    x0 = np.zeros(n)
    return f, h, L, x0


# ---------------------------------------------------------------------------------------------------------------
# Logistic regression instances for the (L0, L1) Frank-Wolfe solvers (accbpg/applications.py:432-701).  The reference
# draws with jax.random; this package draws with NumPy, so the construction is the reference's and the numbers are
# not: ``key`` is an int seed or a np.random.RandomState, used for every draw in the order of the reference's code.
# ---------------------------------------------------------------------------------------------------------------
def toeplitz_matrix(n_features, rho):
    """The n x n matrix rho^|i-j| (accbpg/applications.py:432-434)."""
    idx = np.arange(n_features)
    return rho ** np.abs(idx[:, None] - idx[None, :])


def _rng_of(key):
    return key if isinstance(key, np.random.RandomState) else np.random.RandomState(int(key))


def _correlated_rows(rng, n_samples, n_features, rho):
    """Z L^T with Z ~ N(0, I) and L the lower Cholesky factor of toeplitz_matrix(n_features, rho)."""
    chol = np.linalg.cholesky(toeplitz_matrix(n_features, rho))
    return rng.standard_normal((n_samples, n_features)) @ chol.T


def _row_norm_constants(X):
    """(L, L1) = (max row norm squared, max row norm)"""
    L1 = np.max(np.linalg.norm(X, axis=1))
    return L1 ** 2, L1


def L0L1_FW_log_reg(key, n_samples, n_features, ball_constrnt_radius, solution_spread_radius_btm=0.91,
                    solution_spread_radius_up=0.96, noise=0.0, rho=0.98):
    """The older generator (accbpg/applications.py:437-499): Toeplitz-correlated Gaussian rows, column j scaled by
    3^j, labels sign(X w + noise * N(0, 1)) (0 counted as +1) for a w at 0.91 to 0.96 of the radius from the origin,
    x0 = 1e-6 in every entry.  Returns f, h = SquaredL2Norm(), L, L0 = 1e-9, L1, x0 with L1 the largest row norm and
    L = L1^2.  ``key`` is an int seed or a RandomState and the draws are NumPy's (rows, direction, radius, noise), so
    the construction is the reference's and the numbers are not."""
    rng = _rng_of(key)
    x0 = np.zeros(n_features) + 1e-6
    assert np.linalg.norm(x0, 2) <= ball_constrnt_radius
    assert np.linalg.norm(x0, np.inf) <= ball_constrnt_radius
    X = _correlated_rows(rng, n_samples, n_features, rho)
    X = X * (3.0 ** np.arange(n_features))[None, :]
    direction = rng.standard_normal(n_features)
    direction /= np.linalg.norm(direction)
    true_omega = rng.uniform(ball_constrnt_radius * solution_spread_radius_btm,
                             ball_constrnt_radius * solution_spread_radius_up) * direction
    print("radius is", ball_constrnt_radius)
    print("true omega radius is", float(np.linalg.norm(true_omega, 2)))
    assert np.linalg.norm(true_omega, 2) <= ball_constrnt_radius
    assert np.linalg.norm(true_omega, np.inf) <= ball_constrnt_radius
    y = np.sign(X @ true_omega + noise * rng.standard_normal(n_samples))
    y = np.where(y == 0, 1.0, y)
    print("ratio positive labels:", float(np.sum(y == 1) / y.shape[0]))
    L, L1 = _row_norm_constants(X)
    return LogisticRegression(X, y), SquaredL2Norm(), L, 1e-9, L1, x0


def hard_FW_log_reg_jax(key, n_samples, n_features, radius=1.0, domain="l1", k_sparse=5, rho=0.95, col_scale=10.0,
                        flip_y=0.0, margin=0.5, class_bias=0.0, x0_mode="center", noise=0.01):
    """An ill-conditioned logistic regression instance on a norm ball or the simplex (accbpg/applications.py:502-658):
    Toeplitz-correlated Gaussian rows, columns scaled by col_scale^linspace(0, 1, n), a planted vector in the domain
    (``domain`` "l1" or "simplex": k_sparse positive entries of sum radius; "linf": +-radius; anything else, "l2": on
    the sphere), labels sign(margin * X w + class_bias + noise * N(0, 1)) with a fraction flip_y flipped and 0 counted
    as +1, x0 the origin or (x0_mode other than "center", "l1" / "simplex" only) a vertex.  Returns f, h, L, L0 = 1e-12,
    L1, x0, X, y with L1 the largest row norm and L = L1^2.  ``key`` is an int seed or a RandomState and the draws are
    NumPy's, in the order of the reference's code, so the construction is the reference's and the numbers are not."""
    rng = _rng_of(key)
    X = _correlated_rows(rng, n_samples, n_features, rho)
    X = X * (col_scale ** np.linspace(0, 1, n_features))[None, :]
    if domain in ("l1", "simplex"):
        true_omega = np.zeros(n_features)
        supp = rng.choice(n_features, size=min(k_sparse, n_features), replace=False)
        vals = rng.uniform(0.5, 1.0, size=supp.shape[0])
        true_omega[supp] = vals / np.sum(np.abs(vals)) * radius
        if domain == "simplex":
            true_omega = np.abs(true_omega)
            true_omega = true_omega / np.sum(true_omega) * radius
    elif domain == "linf":
        true_omega = rng.choice(np.array([-1.0, 1.0]), size=n_features) * radius
    else:
        v = rng.standard_normal(n_features)
        true_omega = radius * (v / (np.linalg.norm(v, 2) + 1e-12))
    logits = margin * (X @ true_omega) + class_bias
    y = np.sign(logits + noise * rng.standard_normal(n_samples))
    if flip_y > 0:
        y = np.where(rng.uniform(size=n_samples) < flip_y, -y, y)
    y = np.where(y == 0, 1.0, y)
    x0 = np.zeros(n_features)
    if domain in ("l1", "simplex") and x0_mode != "center":
        x0[rng.randint(0, n_features)] = radius
    L, L1 = _row_norm_constants(X)
    return LogisticRegression(X, y), SquaredL2Norm(), L, 1e-12, L1, x0, X, y


def load_a9a_data(path, bias=True):
    """(X, y) of a LIBSVM file such as a9a (accbpg/applications.py:661-672) through this package's load_libsvm_file:
    the dense feature matrix, a column of ones appended when ``bias``, and the labels mapped to -1 (label <= 0) / +1."""
    X_sparse, y = load_libsvm_file(path)
    X = X_sparse.toarray()
    if bias:
        X = np.hstack([X, np.ones((X.shape[0], 1))])
    return X, np.where(y <= 0, -1, 1)


def L0L1_FW_log_reg_a9a(ball_constrnt_radius, path):
    """Logistic regression on a LIBSVM file for the (L0, L1) Frank-Wolfe solvers (accbpg/applications.py:675-701): the
    columns of load_a9a_data(path) are standardised in place with their mean and population standard deviation -- a
    column of zero variance, the bias among them, keeps the scale 1 and becomes 0 --, x0 is drawn from
    np.random.uniform(-0.5, 0.5, n) (the global generator, as in the reference) and scaled into the l2 and the
    l-infinity ball of the given radius.  Returns f, h = SquaredL2Norm(), L, L0 = 1e-9, L1, x0."""
    X, y = load_a9a_data(path=path)
    X = X.astype(np.float64, copy=False)
    mean, std = X.mean(axis=0), X.std(axis=0)
    std[std == 0.0] = 1.0
    X -= mean
    X /= std
    n_features = X.shape[1]
    x0 = np.random.uniform(low=-0.5, high=0.5, size=n_features)
    x0 = x0 / max(np.linalg.norm(x0, 2) / ball_constrnt_radius, np.linalg.norm(x0, np.inf) / ball_constrnt_radius, 1.0)
    assert np.linalg.norm(x0, 2) <= ball_constrnt_radius
    assert np.linalg.norm(x0, np.inf) <= ball_constrnt_radius
    L, L1 = _row_norm_constants(X)
    return LogisticRegression(X, y), SquaredL2Norm(), L, 1e-9, L1, x0
