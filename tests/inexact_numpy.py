"""NumPy restatement of the reference's inexact-oracle path (accbpg/algorithms.py:593-777; accbpg/applications.py:
209-295; accbpg/utils.py:252-295; accbpg/functions_lmo.py:54-102; accbpg/functions.py:738-759), for the CPU tests: it
reproduces tests/golden/inexact.npz, written by the real reference (tools/gen_golden_inexact.py).  The objective and
the Burg kernel are the restatements of oracle/np_oracle.py.  Each solver also returns its L after every outer
iteration (the reference prints it, and AIBM records it nowhere else)."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.np_oracle import BurgSimplexOracle, PoissonOracle  # noqa: E402


class SquaredL2Norm:
    def extra_Psi(self, x):
        return 0

    def gradient(self, x):
        return x

    def divergence(self, x, y):
        xy = x - y
        return 0.5 * np.vdot(xy, xy)

    def prox_map(self, g, L):
        return -(1 / L) * g

    def div_prox_map(self, y, g, L):
        return y - (1 / L) * g


def random_point_on_simplex(n, radius=1, center=False):
    if center:
        return np.ones(n) / n
    rand_nums = np.random.uniform(low=0.01, high=radius, size=(n - 1,))
    rand_nums.sort()
    return np.diff(np.concatenate([[0], rand_nums, [radius]]))


def edge_point_on_simplex(edge_index, n, radius=1, tol=1e-5):
    x = np.zeros(n) + tol
    x[edge_index] = radius - tol * (n - 1)
    return x


def get_random_float(var=1):
    if var == 0:
        return 0
    assert var > 0, 'The range must be positive.'
    val = var * np.random.random_sample()
    assert val > 0
    return val


def get_random_vector(size, range=1):
    if range == 0:
        return np.zeros(size)
    assert range > 0, 'The range must be positive.'
    vec = range * np.random.random_sample(size=size)
    assert vec.min() > 0
    return vec


def simplex_instance(m, n, noise, normalizeA, solution):
    A = np.random.rand(m, n)
    if normalizeA:
        A = A / A.sum(axis=0)
    b = np.dot(A, solution) + noise * (np.random.rand(m))
    assert b.min() > 0, "need b > 0 for nonnegative regression."
    return A, b


def Poisson_regr_simplex_acc(m, n, noise=0.01, normalizeA=True):
    x0 = random_point_on_simplex(n, center=False)
    solution = random_point_on_simplex(n, center=False)
    A, b = simplex_instance(m, n, noise, normalizeA, solution)
    return PoissonOracle(A, b), [BurgSimplexOracle(eps=1e-7), SquaredL2Norm()], np.abs(b).sum(), x0


PLACEMENTS = ('x0_center_sol_center', 'x0_edge_sol_edge', 'x0_edge_sol_center', 'x0_center_sol_edge')


def Poisson_regr_simplex(m, n, noise=0.01, normalizeA=True):
    out = {}
    for key in PLACEMENTS:
        x0_edge, sol_edge = key.startswith('x0_edge'), key.endswith('sol_edge')
        x0 = edge_point_on_simplex(np.random.randint(n), n) if x0_edge else random_point_on_simplex(n, center=True)
        if sol_edge:
            solution = edge_point_on_simplex(np.random.randint(n), n)
        else:                           # the centre when x0 sits on an edge, a random point when x0 is the centre
            solution = random_point_on_simplex(n, center=x0_edge)
        A, b = simplex_instance(m, n, noise, normalizeA, solution)
        out[key] = (PoissonOracle(A, b), b.sum(), solution, x0)
    return BurgSimplexOracle(), out


def lmo_l2_ball_positive_orthant(radius, center=None, epsilon=0.0):
    def f(g):
        g = np.asarray(g)
        center_p = np.zeros_like(g) if center is None else np.asarray(center)
        assert center_p.shape == g.shape, "Shape mismatch between g and center"
        mask = g < 0
        if not np.any(mask):
            return np.maximum(center_p, epsilon)
        g_neg = g[mask]
        direction = np.zeros_like(g)
        direction[mask] = -g_neg / np.linalg.norm(g_neg)
        s = np.maximum(center_p + radius * direction, epsilon)
        assert np.all(s >= epsilon), "Output violates epsilon-nonnegativity"
        assert np.linalg.norm(s - center_p) <= radius + 1e-8, "Output outside L2 ball"
        return s
    return f


def AIBM(f, h, L, x0, gamma, maxitrs, epsilon=1e-14, noise=0):
    """-> (x, F, G, Lk)"""
    F, G, Lk = np.zeros(maxitrs), np.zeros(maxitrs), np.zeros(maxitrs)
    p = 2
    x = z = np.ones(x0.shape[0]) * h.prox_map(np.zeros(x0.shape[0]), 1)
    delta = get_random_float(noise)
    fx, g = f.func_grad(x, flag=2)
    while True:
        alpha = 1 / L
        y = h.prox_map(g, 1)
        if f(y) <= fx + np.dot(g, y - x) + L * h.divergence(y, x) + epsilon + delta:
            break
        L = L * 2
    B = A = alpha
    xi_grad = alpha * f.gradient(x)
    F[0] = fx + h.extra_Psi(x)
    G[0] = Lk[0] = L
    for k in range(1, maxitrs):
        L /= 2
        delta = get_random_float(noise)
        while True:
            alpha = (1 / L) * (1 + k / (2 * p)) ** ((p - 1) * (gamma - 1))
            B = (L * alpha ** gamma) ** (1 / (gamma - 1))
            x = (alpha / B) * z + (1 - alpha / B) * y
            grad_x = f.gradient(x)
            xi_grad += alpha * grad_x
            z_k = h.prox_map(xi_grad, 1)
            w = alpha / B * z_k + (1 - alpha / B) * y
            fx = f(x)
            if f(w) <= fx + np.dot(grad_x, w - x) + L * h.divergence(w, x) + delta:
                break
            xi_grad -= alpha * grad_x
            L = L * 2
        F[k] = fx + h.extra_Psi(x)
        Lk[k] = L
        A += alpha
        y = B / A * w + (1 - B / A) * y
        z = z_k
        if abs(F[k] - F[k - 1]) < 1e-9:
            break
    return x, F[0:k + 1], G[0:k + 1], Lk[0:k + 1]


def _fgm(f, h, L, x_k, F0, maxitrs, epsilon, draw, noisy_oracle):
    """The loop AdaptFGM and UniversalGM share: `draw()` once per k; noisy_oracle: the draw shifts the gradient and
    f(y) and the test compares with f(y) (UniversalGM), else it is added to the test and f(x_k) enters (AdaptFGM)."""
    F, G = np.zeros(maxitrs), np.zeros(maxitrs)
    F[0], G[0] = F0, L
    u_k = np.ones(x_k.shape)
    A_k = 0
    for k in range(1, maxitrs):
        if noisy_oracle:
            r = draw()
            L /= 2
        else:
            L /= 2
            r = draw()
        while True:
            alpha = (1 + math.sqrt(1 + 4 * L * A_k)) / (2 * L)
            A = L * alpha ** 2
            y = (alpha * u_k + A_k * x_k) / A
            g_y = f.gradient(y)
            if noisy_oracle:
                g_y += r
            u = h.div_prox_map(u_k, g_y * alpha, 1)
            x = (alpha * u + A_k * x_k) / A
            if noisy_oracle:
                base, slack = f(y) + r, 0
            else:
                base, slack = f(x_k), r
            if f(x) <= base + np.sum(g_y * (x - y)) + L * h.divergence(x, y) + slack:
                A_k, u_k, x_k = A, u, x
                break
            L = L * 2
            if L is None or math.isinf(L):
                raise ValueError("L cannot be None or infinity")
        F[k] = f(x_k) + h.extra_Psi(x_k)
        G[k] = L
        if abs(F[k] - F[k - 1]) < epsilon:
            break
    return x_k, F[0:k + 1], G[0:k + 1], G[0:k + 1].copy()


def AdaptFGM(f, h, L, x0, maxitrs, epsilon=1e-14, noise=0):
    """-> (x, F, G, Lk)"""
    x_k = np.ones(x0.shape)
    return _fgm(f, h, L, x_k, f(x_k) + h.extra_Psi(x_k), maxitrs, epsilon, lambda: get_random_float(noise), False)


def UniversalGM(f, h, L, x0, maxitrs, epsilon=1e-14, noise_level=0):
    """-> (x, F, G, Lk)"""
    x_k = np.copy(x0)
    draw = (lambda: np.random.rand() * noise_level) if noise_level > 0 else (lambda: 0)
    return _fgm(f, h, L, x_k, f(x_k) + h.extra_Psi(x_k), maxitrs, epsilon, draw, True)
