"""Plain-torch restatement of the rest of the gyrogroup and of the Riemannian metric of the Poincare ball at k = -1 (math_.py:558-589
mobius_sub, :678-744 mobius_coadd, :747-779 mobius_cosub, :1139-1185 geodesic_unit, :355-383 lambda_x, :386-430 inner, :433-472 norm,
:1816-1845 egrad2rgrad, :1848-1874 sproj, :1877-1905 inv_sproj), for any dtype: the yardstick of tests/test_gpu_gyro_ops.py, which
tests/test_gyro_ops_host.py holds to the reference's own recorded outputs (tests/golden/gyro_ops.npz).

Written from the formulas, clamp by clamp and in the reference's order of operations, on the pieces of tests/tangent_ref.py (the clamped
tanh, lambda_x, mobius_add).  Two differences from the reference, the library's:
    inner with keepdim=False returns one value per row, shape x.shape[:-1]; the reference's product of lambda_x^2 (..., 1) with a sum of
    shape (...) broadcasts the rows against each other there.  With keepdim=True the two agree.
    sproj and inv_sproj use inv_r = 1 for the reference's sqrt(|k| + 1e-15).

The second half restates the BACKWARD of every function by hand, without autograd -- the formulas the kernels evaluate (csrc/rowops.h) --:
tests/test_gyro_ops_host.py holds them to autograd of the first half in fp64.  Nothing flows through a clamp that holds, and the
gradient of a Euclidean norm at exactly 0 is 0.  Values and gradients of one-value-per-row functions are carried as (..., 1) there.
"""
import torch

from tangent_ref import EPS, _conformal, _dot, _lambda, _norm, _tanh, _tanh_prime, _where, mobius_add_bwd, mobius_add_ref


def _per_row(o, keepdim):
    return o if keepdim else o.squeeze(-1)


def mobius_sub_ref(x, y):
    return mobius_add_ref(x, -y)


def mobius_coadd_ref(x, y):
    x2, y2 = _dot(x, x), _dot(y, y)
    return ((1 - y2) * x + (1 - x2) * y) / (1 - x2 * y2).clamp_min(EPS)


def mobius_cosub_ref(x, y):
    return mobius_coadd_ref(x, -y)


def geodesic_unit_ref(t, x, u):
    n = _norm(u).clamp_min(EPS)
    return mobius_add_ref(x, _tanh(t / 2.0) * (u / n))


def lambda_x_ref(x, keepdim=False):
    return _per_row(_lambda(x), keepdim)


def inner_ref(x, u, v, keepdim=False):
    return _per_row(_lambda(x) ** 2 * _dot(u, v), keepdim)


def norm_ref(x, u, keepdim=False):
    return _per_row(_lambda(x) * _norm(u), keepdim)


def egrad2rgrad_ref(x, grad):
    return grad / _lambda(x) ** 2


def sproj_ref(h):
    return (1.0 / (1.0 + h[..., -1:])) * h[..., :-1]


def inv_sproj_ref(x):
    lam = _lambda(x)
    return torch.cat((lam * x, lam - 1.0), dim=-1)


def antipode_ref(x):
    return -x


# ================================================================================================ the backward formulas, by hand
def mobius_sub_bwd(x, y, go):
    dx, dny = mobius_add_bwd(x, -y, go)
    return dx, -dny


def _coadd_bwd(x, y, go, sy):
    y = sy * y
    x2, y2 = _dot(x, x), _dot(y, y)
    A, B, draw = 1 - y2, 1 - x2, 1 - x2 * y2
    rD = 1 / draw.clamp_min(EPS)
    m, dN = (A * x + B * y) * rD, go * rD
    dD = _where(draw >= EPS, -_dot(go, m) * rD)
    dA, dB = _dot(dN, x), _dot(dN, y)
    return A * dN + 2 * (-dB - y2 * dD) * x, sy * (B * dN + 2 * (-dA - x2 * dD) * y)


def mobius_coadd_bwd(x, y, go):
    return _coadd_bwd(x, y, go, 1.0)


def mobius_cosub_bwd(x, y, go):
    return _coadd_bwd(x, y, go, -1.0)


def geodesic_unit_bwd(t, x, u, go):
    """(dL/dt per row, dL/dx, dL/du)."""
    raw = _norm(u)
    n = raw.clamp_min(EPS)
    th = _tanh(t / 2.0)
    tp = _tanh_prime(t / 2.0, th)
    f = th / n
    dx, ds = mobius_add_bwd(x, f * u, go)
    gf = _dot(ds, u)
    return 0.5 * gf * tp / n, dx, f * ds + _where(raw >= EPS, -gf * th / (n * n * n)) * u


def lambda_x_bwd(x, g):
    c, cp = _conformal(_dot(x, x))
    return (-4 * g / (c * c) * cp * x,)


def inner_bwd(x, u, v, g):
    c, cp = _conformal(_dot(x, x))
    s = g * 4 / (c * c)
    return -16 * g * _dot(u, v) / (c * c * c) * cp * x, s * v, s * u


def norm_bwd(x, u, g):
    c, cp = _conformal(_dot(x, x))
    n = _norm(u)
    s = _where(n > 0, 2 * g / (c * n.clamp_min(1e-300)))
    return -4 * g * n / (c * c) * cp * x, s * u


def egrad2rgrad_bwd(x, grad, go):
    c, cp = _conformal(_dot(x, x))
    return _dot(go, grad) * c * cp * x, 0.25 * c * c * go


def sproj_bwd(h, go):
    f = 1 / (1 + h[..., -1:])
    return (torch.cat((f * go, -f * f * _dot(go, h[..., :-1])), dim=-1),)


def inv_sproj_bwd(x, go):
    c, cp = _conformal(_dot(x, x))
    glam = _dot(go[..., :-1], x) + go[..., -1:]
    return (2 / c * go[..., :-1] - 4 * glam / (c * c) * cp * x,)
