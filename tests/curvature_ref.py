"""Plain-torch restatement of the 25 row-wise functions of math_.py with the curvature explicit, k < 0, for any dtype: the yardstick of
tests/test_gpu_ball_curvature.py, which tests/test_ball_curvature_host.py holds to the reference's own recorded outputs at k = -0.5 and
k = -2 (tests/golden/curvature.npz) and, at k = -1, to tests/tangent_ref.py, tests/gyro_ref.py and tests/dist_ref.py.

Written from the formulas, clamp by clamp and in the reference's order of operations:
    tanh clamps its argument to +-15, artanh to +-(1 - 1e-7)                                          :51-59
    tan_k(x) = tanh(sqrt(-k) x) / sqrt(-k), artan_k(x) = artanh(sqrt(-k) x) / sqrt(-k)                :190-262
    lambda_x = 2 / max(1 + k |x|^2, 1e-15)                                                            :382-383
    mobius_add(x, y) = ((1 - 2k xy - k y2) x + (1 + k x2) y) / max(1 - 2k xy + k^2 x2 y2, 1e-15)      :536-555
with the library's differences: artanh is 0.5 (log1p(x) - log1p(-x)) (tests/tangent_ref.py), inner with keepdim=False returns one value
per row, and sproj / inv_sproj use sqrt(-k) for the reference's sqrt(|k| + 1e-15).

``k`` is a negative number.  Results of one value per row have the shape x.shape[:-1], or (..., 1) with keepdim.
"""
import math

import torch

EPS = 1e-15
TANH_CLAMP = 15.0
ARTANH_TOP = 1 - 1e-7


def _dot(a, b):
    return (a * b).sum(dim=-1, keepdim=True)


def _norm(a):
    return a.norm(dim=-1, p=2, keepdim=True)


def _per_row(o, keepdim):
    return o if keepdim else o.squeeze(-1)


def _tanh(x):
    return x.clamp(-TANH_CLAMP, TANH_CLAMP).tanh()


def _artanh(x):
    x = x.clamp(-ARTANH_TOP, ARTANH_TOP)
    return 0.5 * (torch.log1p(x) - torch.log1p(-x))


def tan_k(x, k):
    s = math.sqrt(-k)
    return (1 / s) * _tanh(x * s)


def artan_k(x, k):
    s = math.sqrt(-k)
    return (1 / s) * _artanh(x * s)


def _lambda(x, k):
    return 2 / (1 + k * _dot(x, x)).clamp_min(EPS)


def project(x, k, eps=4e-3):
    """eps: the reference's fp32 default, which the kernels use whatever the dtype here."""
    maxnorm = (1 - eps) / math.sqrt(-k)
    n = _norm(x).clamp_min(EPS)
    return torch.where(n > maxnorm, x / n * maxnorm, x)


def lambda_x(x, k, keepdim=False):
    return _per_row(_lambda(x, k), keepdim)


def inner(x, u, v, k, keepdim=False):
    return _per_row(_lambda(x, k) ** 2 * _dot(u, v), keepdim)


def norm(x, u, k, keepdim=False):
    return _per_row(_lambda(x, k) * _norm(u), keepdim)


def mobius_add(x, y, k):
    x2, y2, xy = _dot(x, x), _dot(y, y), _dot(x, y)
    num = (1 - 2 * k * xy - k * y2) * x + (1 + k * x2) * y
    return num / (1 - 2 * k * xy + k ** 2 * x2 * y2).clamp_min(EPS)


def mobius_sub(x, y, k):
    return mobius_add(x, -y, k)


def gyration(a, b, u, k):
    a2, b2, ab, au, bu = _dot(a, a), _dot(b, b), _dot(a, b), _dot(a, u), _dot(b, u)
    k2 = k ** 2
    A = -k2 * au * b2 - k * bu + 2 * k2 * ab * bu
    B = -k2 * bu * a2 + k * au
    d = 1 - 2 * k * ab + k2 * a2 * b2
    return u + 2 * (A * a + B * b) / d.clamp_min(EPS)


def mobius_coadd(x, y, k):
    x2, y2 = _dot(x, x), _dot(y, y)
    return ((1 + k * y2) * x + (1 + k * x2) * y) / (1 - k ** 2 * x2 * y2).clamp_min(EPS)


def mobius_cosub(x, y, k):
    return mobius_coadd(x, -y, k)


def mobius_scalar_mul(r, x, k):
    n = _norm(x).clamp_min(EPS)
    return tan_k(r * artan_k(n, k), k) * (x / n)


def dist(x, y, k, keepdim=False):
    return _per_row(2.0 * artan_k(_norm(mobius_add(-x, y, k)), k), keepdim)


def dist0(x, k, keepdim=False):
    return _per_row(2.0 * artan_k(_norm(x), k), keepdim)


def geodesic(t, x, y, k):
    return mobius_add(x, mobius_scalar_mul(t, mobius_add(-x, y, k), k), k)


def expmap(x, u, k):
    n = _norm(u).clamp_min(EPS)
    return mobius_add(x, tan_k((_lambda(x, k) / 2.0) * n, k) * (u / n), k)


def expmap0(u, k):
    n = _norm(u).clamp_min(EPS)
    return tan_k(n, k) * (u / n)


def geodesic_unit(t, x, u, k):
    n = _norm(u).clamp_min(EPS)
    return mobius_add(x, tan_k(t / 2.0, k) * (u / n), k)


def logmap(x, y, k):
    sub = mobius_add(-x, y, k)
    n = _norm(sub).clamp_min(EPS)
    return 2.0 * artan_k(n, k) * (sub / (_lambda(x, k) * n))


def logmap0(y, k):
    n = _norm(y).clamp_min(EPS)
    return (y / n) * artan_k(n, k)


def mobius_pointwise_mul(w, x, k):
    xn = _norm(x).clamp_min(EPS)
    wx = w * x
    wn = _norm(wx).clamp_min(EPS)
    res = tan_k(wn / xn * artan_k(xn, k), k) * (wx / wn)
    zero = torch.zeros((), dtype=res.dtype, device=res.device)
    cond = (wx.abs() <= 1e-8).all(dim=-1, keepdim=True)          # the reference's isclose(wx, 0)
    return torch.where(cond, zero, res)


def parallel_transport(x, y, v, k):
    return gyration(y, -x, v, k) * _lambda(x, k) / _lambda(y, k)


def parallel_transport0(y, v, k):
    return v * (1 + k * _dot(y, y)).clamp_min(EPS)


def parallel_transport0back(x, v, k):
    return v / (1 + k * _dot(x, x)).clamp_min(EPS)


def egrad2rgrad(x, grad, k):
    return grad / _lambda(x, k) ** 2


def sproj(h, k):
    return (1.0 / (1.0 + math.sqrt(-k) * h[..., -1:])) * h[..., :-1]


def inv_sproj(x, k):
    lam = _lambda(x, k)
    return torch.cat((lam * x, 1.0 / math.sqrt(-k) * (lam - 1.0)), dim=-1)


def antipode(x, k):
    return -x


# name: (function, operand names in the method's order, one value per row?)
FUNCTIONS = {
    "project": (project, ("x",), False), "expmap0": (expmap0, ("u",), False), "logmap0": (logmap0, ("y",), False),
    "dist0": (dist0, ("x",), True), "sproj": (sproj, ("h",), False), "inv_sproj": (inv_sproj, ("x",), False),
    "mobius_add": (mobius_add, ("x", "y"), False), "mobius_sub": (mobius_sub, ("x", "y"), False),
    "mobius_coadd": (mobius_coadd, ("x", "y"), False), "mobius_cosub": (mobius_cosub, ("x", "y"), False), "dist": (dist, ("x", "y"), True),
    "logmap": (logmap, ("x", "y"), False), "expmap": (expmap, ("x", "u"), False),
    "mobius_scalar_mul": (mobius_scalar_mul, ("r", "x"), False), "mobius_pointwise_mul": (mobius_pointwise_mul, ("w", "x"), False),
    "geodesic": (geodesic, ("t", "x", "y"), False), "geodesic_unit": (geodesic_unit, ("t", "x", "u"), False),
    "gyration": (gyration, ("a", "b", "u"), False), "parallel_transport": (parallel_transport, ("x", "y", "v"), False),
    "parallel_transport0": (parallel_transport0, ("y", "v"), False), "parallel_transport0back": (parallel_transport0back, ("x", "v"), False),
    "norm": (norm, ("x", "u"), True), "egrad2rgrad": (egrad2rgrad, ("x", "grad"), False), "lambda_x": (lambda_x, ("x",), True),
    "inner": (inner, ("x", "u", "v"), True),
}
# The exponents of s = sqrt(c) on each operand and on the result (docs/history/curvature.md): f_c(a_0, ...) = s^eo f_1(s^e0 a_0, ...)
EXPONENTS = {
    "project": ((1,), -1), "expmap0": ((1,), -1), "logmap0": ((1,), -1), "dist0": ((1,), -1), "sproj": ((1,), -1), "inv_sproj": ((1,), -1),
    "mobius_add": ((1, 1), -1), "mobius_sub": ((1, 1), -1), "mobius_coadd": ((1, 1), -1), "mobius_cosub": ((1, 1), -1), "dist": ((1, 1), -1),
    "logmap": ((1, 1), -1), "expmap": ((1, 1), -1), "mobius_scalar_mul": ((0, 1), -1), "mobius_pointwise_mul": ((0, 1), -1),
    "geodesic": ((0, 1, 1), -1), "geodesic_unit": ((1, 1, 0), -1), "gyration": ((1, 1, 0), 0), "parallel_transport": ((1, 1, 0), 0),
    "parallel_transport0": ((1, 0), 0), "parallel_transport0back": ((1, 0), 0), "norm": ((1, 0), 0), "egrad2rgrad": ((1, 0), 0),
    "lambda_x": ((1,), 0), "inner": ((1, 0, 0), 0),
}
