"""Linear minimisation oracles (accbpg/functions_lmo.py): the simplex (:137-160), whose vertex that minimises <g, s>
is returned with 1e-15 in every other entry as the reference does (so that Burg divergences from it stay finite),
the l2 and l-infinity balls (:16-51, :106-134) for vector or n x r matrix gradients, and the l2 ball cut by the
(strictly) positive orthant (:54-102).  NumPy in, NumPy out; CUDA tensor in, CUDA tensor out."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .functions import _Workspace, _ptr, _stream, from_dev, to_dev, vec_argminmax, vec_dot, vec_vertex


LMO_L2, LMO_LINF, LMO_SIMPLEX = 0, 1, 2      # the lmo_kind of accbpg_fw_direction


class _Lmo:
    """An oracle of this module: the callable g -> s it has always been, which also says what it is -- ``kind`` (one of
    LMO_L2, LMO_LINF, LMO_SIMPLEX), ``radius`` and ``center`` (a _Center, None for the simplex) -- so that a solver can
    hand the whole direction step to ``fw_direction``."""

    def __init__(self, call, kind, radius, center):
        self._call, self.kind, self.radius, self.center = call, kind, radius, center

    def __call__(self, g):
        return self._call(g)


def fw_direction(lmo, g, x):
    """(s, d, gg, slope, dd, index, dist) for an oracle of this module: s = lmo(g), d = s - x, gg = sum g^2,
    slope = <g, d>, dd = sum d^2, the simplex vertex's index and the l2 ball's ||s - c|| (0.0 for the other oracles and
    for the ball's centre), in one call with one read-back (accbpg_fw_direction).  g and x are CUDA tensors of the same
    shape; s and d have that shape.  Entry by entry and sum by sum the result has the bits of lmo(g),
    vec_axpby(1, s, -1, x) and vec_dot on them."""
    assert isinstance(lmo, _Lmo), "fw_direction: not an oracle of functions_lmo"
    gd, xd = g.contiguous(), x.contiguous()
    assert gd.shape == xd.shape, "fw_direction: g and x not same shape."
    kind, cd, val = (0, None, 0.0) if lmo.center is None else lmo.center.args(gd)
    n = gd.numel()
    s, d = torch.empty_like(gd), torch.empty_like(gd)
    out, idx = (C.c_double * 5)(), (C.c_int64 * 1)()
    with torch.cuda.device(gd.device):
        ws = _Workspace.get(n, gd.device)
        rc = _lib.load().accbpg_fw_direction(_ptr(gd), _ptr(xd), lmo.kind, kind, _ptr(cd), val, float(lmo.radius), n,
                                             _ptr(s), _ptr(d), out, idx, _ptr(ws), _stream())
    _lib.check(rc, "accbpg_fw_direction", "Solution does not lie on ball boundary")
    return s, d, np.float64(out[0]), np.float64(out[1]), np.float64(out[2]), int(idx[0]), out[3]


def lmo_simplex(radius=1):
    """Returns g -> s with s[i] = 1e-15 and s[first argmin g] = radius (NumPy in, NumPy out; CUDA
    tensor in, CUDA tensor out: first-index argmin and the fill run on the device)."""
    def vertex(g):
        gd, was_np = to_dev(g)
        imin, _, _, _ = vec_argminmax(gd)
        return from_dev(vec_vertex(imin, radius, 1e-15, gd.numel(), gd.device), was_np)
    return _Lmo(vertex, LMO_SIMPLEX, radius, None)


class _Center:
    """The centre of a ball as the kernels take it: (kind 0, scalar) for None or a scalar, (kind 1, device array
    broadcast to the gradient's shape) otherwise; the device copy is made once per shape and device."""

    def __init__(self, center):
        self.center = center
        self.scalar = center is None or np.ndim(center) == 0
        self._cache = {}

    def args(self, gd):
        if self.scalar:
            return 0, None, 0.0 if self.center is None else float(self.center)
        key = (tuple(gd.shape), gd.device)
        cd = self._cache.get(key)
        if cd is None:
            if isinstance(self.center, torch.Tensor):
                cd = torch.broadcast_to(self.center.to(device=gd.device, dtype=torch.float64), gd.shape).contiguous()
            else:
                cd = torch.from_numpy(np.array(
                    np.broadcast_to(np.asarray(self.center, dtype=np.float64), tuple(gd.shape)))).to(gd.device)
            self._cache = {key: cd}
        return 1, cd, 0.0

    def full(self, gd):
        kind, cd, val = self.args(gd)
        return cd.clone() if kind == 1 else torch.full(gd.shape, val, dtype=torch.float64, device=gd.device)


def lmo_l2_ball(radius, center=None):
    """Returns g -> s = c - radius*g/||g||_F, the minimiser of <g, s> over {||s - c|| <= radius}; the centre itself
    when ||g|| < 1e-10.  Asserts | ||s - c|| - radius | <= 1e-10 with the norm taken in the same launch."""
    cen = _Center(center)

    def f(g):
        gd, was_np = to_dev(g)
        g_norm = np.sqrt(np.float64(vec_dot(gd, gd)))
        if g_norm < 1e-10:
            return from_dev(cen.full(gd), was_np)
        kind, cd, val = cen.args(gd)
        n = gd.numel()
        out = torch.empty_like(gd)
        dist = C.c_double(0.0)
        with torch.cuda.device(gd.device):
            ws = _Workspace.get(n, gd.device)
            rc = _lib.load().accbpg_lmo_l2_ball(_ptr(gd), kind, _ptr(cd), val, float(radius), float(g_norm), n,
                                                _ptr(out), C.byref(dist), _ptr(ws), _stream())
        _lib.check(rc, "accbpg_lmo_l2_ball", "Solution does not lie on ball boundary")
        return from_dev(out, was_np)

    return _Lmo(f, LMO_L2, radius, cen)


def lmo_linf_ball(radius, center=None):
    """Returns g -> s = c - radius*sign(g) (sign(0) = 0), a vertex of {||s - c||_inf <= radius}.  The centre may be
    None, a scalar or an array of the gradient's shape."""
    cen = _Center(center)

    def f(g):
        gd, was_np = to_dev(g)
        kind, cd, val = cen.args(gd)
        out = torch.empty_like(gd)
        with torch.cuda.device(gd.device):
            rc = _lib.load().accbpg_lmo_linf_ball(_ptr(gd), kind, _ptr(cd), val, float(radius), gd.numel(), _ptr(out),
                                                  _stream())
        _lib.check(rc, "accbpg_lmo_linf_ball")
        return from_dev(out, was_np)

    return _Lmo(f, LMO_LINF, radius, cen)


def lmo_l2_ball_positive_orthant(radius, center=None, epsilon=0.0):
    """Returns g -> s = max(c + radius*d, epsilon) with d = -g/||g[g < 0]|| on the negative entries of g and 0
    elsewhere: the minimiser of <g, s> over the l2 ball moved along the coordinates that pay, then lifted to
    s >= epsilon.  A gradient with no negative entry gives max(c, epsilon) and, as in the reference, skips both
    assertions (s >= epsilon, ||s - c|| <= radius + 1e-8).  The centre is None (zeros) or an array of the gradient's
    shape.  The masked norm, the output and the two checked quantities come from the device with one read-back; g is
    not copied to the host."""
    cache = {}

    def f(g):
        gd, was_np = to_dev(g)
        cd = None
        if center is not None:
            assert tuple(np.shape(center)) == tuple(gd.shape), "Shape mismatch between g and center"
            key = (tuple(gd.shape), gd.device)
            cd = cache.get(key)
            if cd is None:
                cd, _ = to_dev(center)
                cd = cd.to(gd.device)
                cache.clear()
                cache[key] = cd
        n = gd.numel()
        out = torch.empty_like(gd)
        info = (C.c_double * 3)()
        with torch.cuda.device(gd.device):
            ws = _Workspace.get(n, gd.device)
            rc = _lib.load().accbpg_lmo_l2_ball_pos(_ptr(gd), _ptr(cd), float(radius), float(epsilon), n, _ptr(out), info,
                                                    _ptr(ws), _stream())
        _lib.check(rc, "accbpg_lmo_l2_ball_pos")
        return from_dev(out, was_np)

    return f
