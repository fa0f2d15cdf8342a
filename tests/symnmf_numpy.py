"""NumPy restatement of the reference's symmetric-NMF path (accbpg/functions.py:493-577, 738-759, 908-976;
accbpg/functions_lmo.py:16-51, 106-134; accbpg/algorithms_fw.py:6-75, 210-247; accbpg/applications.py:330-415), for
the CPU tests: it reproduces tests/golden/symnmf.npz, written by the real reference.  `order` switches the summation
order of M X (0: M @ X as the reference, 1: the sum of two half-depth products), which measures how far the
reference's own trajectories move under a change of rounding alone."""
import math

import numpy as np


class FrobeniusSymLoss:
    def __init__(self, M, X_init, noise_level=None, order=0):
        assert np.allclose(M, M.T), "Matrix M must be symmetric."
        self.M = M
        self.M_norm = np.linalg.norm(M)
        self.noise_level = noise_level
        self.order = order

    def _mx(self, X):
        if self.order == 0:
            return self.M @ X
        k = X.shape[0] // 2
        return self.M[:, :k] @ X[:k] + self.M[:, k:] @ X[k:]

    def __call__(self, x):
        return self.func_grad(x, flag=0)

    def gradient(self, x):
        return self.func_grad(x, flag=1)

    def func_grad(self, X, flag=2):
        noise = 0
        if self.noise_level is not None:
            noise = (np.random.randn(*X.shape) - 0.5) * self.noise_level
        XM = self._mx(X)
        f = 0.5 * (self.M_norm ** 2 + np.linalg.norm(X.T @ X) ** 2) - np.dot(X.ravel(), XM.ravel())
        if flag == 0:
            return f
        g = 2 * (X @ (X.T @ X)) - 2 * XM
        return g + noise if flag == 1 else (f, g + noise)


class SumOf2nd4thPowers:
    upper_bound = None
    clip = False

    def __init__(self, alpha, sigma):
        self.alpha = alpha
        self.sigma = sigma

    def extra_Psi(self, x):
        return 0

    def __call__(self, x):
        norm = np.linalg.norm(x)
        return (self.alpha / 4) * norm ** 4 + self.sigma / 2 * norm ** 2

    def gradient(self, x):
        return (self.sigma + self.alpha * np.linalg.norm(x) ** 2) * x

    def divergence(self, x, y):
        return self(x) - (self(y) + np.sum(self.gradient(y) * (x - y)))

    def solve_cubic(self, c, alpha):
        z = alpha / 3.0
        alpha3 = alpha ** 3
        delta = c ** 2 + 4 * alpha3 * c / 27.0
        sq_delta = np.sqrt(delta)
        b = 0.5 * c + alpha3 / 27.0
        z += np.cbrt(b + 0.5 * sq_delta)
        z += np.cbrt(b - 0.5 * sq_delta)
        return z

    def div_prox_map(self, y, g, L):
        z = self.alpha * np.linalg.norm(y) ** 2 + self.sigma
        y = z * y - (1 / L) * g
        if self.clip:
            y = np.clip(y, 0, self.upper_bound)
        z = self.solve_cubic(self.alpha * np.linalg.norm(y) ** 2, self.sigma)
        return y / z


class SumOf2nd4thPowersPositiveOrthant(SumOf2nd4thPowers):
    clip = True

    def __init__(self, alpha, sigma, upper_bound=None):
        SumOf2nd4thPowers.__init__(self, alpha, sigma)
        self.upper_bound = upper_bound


def lmo_l2_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else np.broadcast_to(center, g.shape)
        g_norm = np.linalg.norm(g)
        if g_norm < 1e-10:
            return c
        s = c - radius * g / g_norm
        assert abs(np.linalg.norm(s - c) - radius) <= 1e-10, "Solution does not lie on ball boundary"
        return s
    return f


def lmo_linf_ball(radius, center=None):
    def f(g):
        c = np.zeros_like(g) if center is None else np.array(center)
        return c - radius * np.sign(g)
    return f


def l2_instance(n, r, ball_center, radius=1.0, on_boundary=True):
    X = np.random.randn(n, r)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    if on_boundary:
        X *= radius
    else:
        X *= radius * np.random.uniform(0, 1, size=(n, 1)) ** (1 / r)
    X += ball_center
    return X.dot(X.T), np.ones((n, r)) * radius + 1e-5 * radius


def linf_instance(n, r, ball_center, radius=1.0, on_boundary=True):
    X = np.random.randn(n, r)
    X /= np.max(np.abs(X))
    if on_boundary:
        X *= radius
    else:
        X *= radius * np.random.uniform(0, 1)
    X += ball_center
    return X @ X.T, np.ones((n, r)) * radius + 1e-5 * radius


def FW_alg_div_step(f, h, L, x0, maxitrs, gamma, lmo, epsilon=1e-14, linesearch=True, ls_ratio=2):
    F, Ls = [], []
    x = np.copy(x0)
    for k in range(maxitrs):
        fx, g = f.func_grad(x)
        F.append(fx)
        s = lmo(g)
        d = s - x
        div = h.divergence(s, x)
        if div == 0:
            div = 1e-6
        gd = np.dot(g.ravel(), d.ravel())
        if 0 < gd <= 1e-6:
            gd = 0.0
        if linesearch:
            L = L / ls_ratio
        while True:
            a = min((-gd / (2 * L * div)) ** (1 / (gamma - 1)), 1.0)
            x1 = x + a * d
            if not linesearch or f.func_grad(x1, flag=0) <= fx + a * gd + a ** gamma * L * div:
                break
            L = L * ls_ratio
        x = x1
        Ls.append(L)
        if k > 0 and abs(F[k] - F[k - 1]) < epsilon:
            break
    return x, np.array(F), np.array(Ls)


def FW_alg_descent_step(f, h, x0, maxitrs, lmo, epsilon=1e-14):
    F = np.zeros(maxitrs)
    x = np.copy(x0)
    fx, g = f.func_grad(x)
    F[0] = fx
    k = 0
    for k in range(1, maxitrs):
        d = lmo(g) - x
        x = x + 2 / (k + 2) * d
        fx, g = f.func_grad(x)
        F[k] = fx
        if abs(F[k] - F[k - 1]) < epsilon or math.sqrt(np.sum(g * g)) < epsilon:
            break
    return x, F[:k + 1]
