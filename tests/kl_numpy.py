"""NumPy restatement of the KL-divergence regression objective and the Shannon-entropy kernels of the reference
(accbpg/functions.py:123-158, 398-490) and of its instance factory (accbpg/applications.py:175-206).

The oracle of the KL tests for shapes that have no golden fixture.  Same operations in the same order as the
reference (separate ufuncs, Python's left-to-right ``sum`` where the reference uses it), so it reproduces
tests/golden/kl.npz to rounding.  The solvers of oracle/np_oracle.py take these objects as they are."""
import numpy as np


def _seq_sum(a):
    return sum(a)


class KLdiv:
    """f(x) = D_KL(Ax, b)."""

    def __init__(self, A, b):
        assert A.shape[0] == b.shape[0], "A and b size not matching"
        self.A, self.b = A, b
        self.m, self.n = A.shape

    def __call__(self, x):
        return self.func_grad(x, 0)

    def gradient(self, x):
        return self.func_grad(x, 1)

    def func_grad(self, x, flag=2):
        assert x.size == self.n, "NonnegRegression: x.size not equal to n."
        Ax = np.dot(self.A, x)
        lg = np.log(Ax / self.b)
        fx = _seq_sum(Ax * lg - Ax + self.b) if flag != 1 else None
        if flag == 0:
            return fx
        g = (lg.reshape(self.m, 1) * self.A).sum(axis=0)
        return g if flag == 1 else (fx, g)


class Shannon:
    """h(x) = sum x log x on x >= 0."""
    lamda = 0

    def __init__(self, delta=1e-20):
        self.delta = delta

    def extra_Psi(self, x):
        return 0

    def divergence(self, x, y):
        assert x.shape == y.shape, "Vectors x and y are of different shapes."
        assert x.min() >= 0 and y.min() >= 0, "Some entries are negative."
        s1 = _seq_sum(x * np.log((x + self.delta) / (y + self.delta)))
        return s1 + (_seq_sum(y) - _seq_sum(x))

    def _g(self, g):
        return g

    def prox_map(self, g, L):
        assert L > 0, "ShannonEntropy prox_map require L > 0."
        return np.exp(-self._g(g) / L - 1)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different sizes."
        assert y.min() >= 0 and L > 0, "Some entries of y are negavie."
        return y * np.exp(-self._g(g) / L)


class ShannonL1(Shannon):
    def __init__(self, lamda=0, delta=1e-20):
        Shannon.__init__(self, delta)
        self.lamda = lamda

    def extra_Psi(self, x):
        return self.lamda * x.sum()

    def _g(self, g):
        return self.lamda + g


class ShannonSimplex(Shannon):
    def prox_map(self, g, L):
        x = Shannon.prox_map(self, g, L)
        return x / _seq_sum(x)

    def div_prox_map(self, y, g, L):
        assert y.shape == g.shape, "Vectors y and g are of different shapes."
        assert y.min() > 0 and L > 0, "prox_map needs positive arguments."
        x = y * np.exp(-g / L)
        return x / _seq_sum(x)


def kl_instance(m, n, noise=0.01, randseed=-1, normalizeA=True):
    """(A, b): legacy global RNG drawn in the order A, x, noise."""
    if randseed > 0:
        np.random.seed(randseed)
    A = np.random.rand(m, n)
    if normalizeA:
        A = A / A.sum(axis=0)
    x = np.random.rand(n)
    b = np.dot(A, x) + noise * (np.random.rand(m) - 0.5)
    assert b.min() > 0, "need b > 0 for nonnegative regression."
    return A, b


def KL_nonneg_regr(m, n, noise=0.01, lamdaL1=0, randseed=-1, normalizeA=True):
    A, b = kl_instance(m, n, noise, randseed, normalizeA)
    return KLdiv(A, b), ShannonL1(lamdaL1), max(A.sum(axis=0)), 0.5 * np.ones(n)
