"""Plain-torch restatement of the tangent maps at a point of the Poincare ball at k = -1 (math_.py:1052-1102 expmap, :1188-1230 logmap,
:978-1049 geodesic, :592-675 gyration, :1669-1813 the three transports), for any dtype: the yardstick of tests/test_gpu_tangent_maps.py,
which tests/test_tangent_maps_host.py holds to the reference's own recorded outputs (tests/golden/tangent_maps.npz).

Written from the formulas, clamp by clamp and in the reference's order of operations:
    tanh clamps its argument to +-15, artanh to +-(1 - 1e-7)                                         :51-59
    lambda_x = 2 / max(1 - |x|^2, 1e-15)                                                             :382-383
    mobius_add(x, y) = ((1 + 2 xy + y2) x + (1 - x2) y) / max(1 + 2 xy + x2 y2, 1e-15)               :536-555
    mobius_scalar_mul(r, x) = tanh(r artanh(n)) x / n, n = max(|x|, 1e-15)                           :853-858
with one difference, the library's: artanh is 0.5 (log1p(x) - log1p(-x)), not 0.5 (log(1 + x) - log(1 - x)).  The two agree to
rounding wherever 1 + x keeps digits of x; below that (|x| < 1e-7 in fp32) the reference's form returns 0 with gradient 0 and this
one x with gradient 1, the analytic limit.

The second half restates the BACKWARD of every map by hand, without autograd -- the formulas the kernels evaluate (csrc/rowops.h) --:
tests/test_tangent_maps_host.py holds them to autograd of the first half in fp64.  Nothing flows through a clamp that holds (torch's
clamp passes the gradient where the bound is met with equality), and the norm's gradient at exactly 0 is 0.
"""
import torch

EPS = 1e-15
TANH_CLAMP = 15.0
ARTANH_TOP = 1 - 1e-7


def _dot(a, b):
    return (a * b).sum(dim=-1, keepdim=True)


def _norm(a):
    return a.norm(dim=-1, p=2, keepdim=True)


def _tanh(x):
    return x.clamp(-TANH_CLAMP, TANH_CLAMP).tanh()


def _artanh(x):
    x = x.clamp(-ARTANH_TOP, ARTANH_TOP)
    return 0.5 * (torch.log1p(x) - torch.log1p(-x))


def _lambda(x):
    return 2 / (1 - _dot(x, x)).clamp_min(EPS)


def mobius_add_ref(x, y):
    x2, y2, xy = _dot(x, x), _dot(y, y), _dot(x, y)
    return ((1 + 2 * xy + y2) * x + (1 - x2) * y) / (1 + 2 * xy + x2 * y2).clamp_min(EPS)


def mobius_scalar_mul_ref(r, x):
    n = _norm(x).clamp_min(EPS)
    return _tanh(r * _artanh(n)) * (x / n)


def expmap_ref(x, u):
    n = _norm(u).clamp_min(EPS)
    return mobius_add_ref(x, _tanh((_lambda(x) / 2.0) * n) * (u / n))


def logmap_ref(x, y):
    sub = mobius_add_ref(-x, y)
    n = _norm(sub).clamp_min(EPS)
    return 2.0 * _artanh(n) * (sub / (_lambda(x) * n))


def geodesic_ref(t, x, y):
    return mobius_add_ref(x, mobius_scalar_mul_ref(t, mobius_add_ref(-x, y)))


def gyration_ref(a, b, u):
    a2, b2, ab, au, bu = _dot(a, a), _dot(b, b), _dot(a, b), _dot(a, u), _dot(b, u)
    A = -au * b2 + bu + 2 * ab * bu
    B = -bu * a2 - au
    d = 1 + 2 * ab + a2 * b2
    return u + 2 * (A * a + B * b) / d.clamp_min(EPS)


def parallel_transport_ref(x, y, v):
    return gyration_ref(y, -x, v) * _lambda(x) / _lambda(y)


def parallel_transport0_ref(y, v):
    return v * (1 - _dot(y, y)).clamp_min(EPS)


def parallel_transport0back_ref(x, v):
    return v / (1 - _dot(x, x)).clamp_min(EPS)


# ================================================================================================ the backward formulas, by hand
def _where(cond, a):
    return torch.where(cond, a, torch.zeros_like(a))


def _conformal(x2):
    """c = max(1 - |x|^2, 1e-15) = 2 / lambda_x and dc / d|x|^2."""
    return (1 - x2).clamp_min(EPS), _where(1 - x2 >= EPS, -torch.ones_like(x2))


def _tanh_prime(arg, t):
    return _where(arg.abs() <= TANH_CLAMP, 1 - t * t)


def _artanh_prime(n):
    return _where(n <= ARTANH_TOP, 1 / ((1 - n) * (1 + n)))


def mobius_add_bwd(x, y, dm):
    x2, y2, xy = _dot(x, x), _dot(y, y), _dot(x, y)
    A, Bc, draw = 1 + 2 * xy + y2, 1 - x2, 1 + 2 * xy + x2 * y2
    rD = 1 / draw.clamp_min(EPS)
    m, dN = (A * x + Bc * y) * rD, dm * rD
    dD = _where(draw >= EPS, -_dot(dm, m) * rD)
    dA, dBc = _dot(dN, x), _dot(dN, y)
    dxy, dx2, dy2 = 2 * dA + 2 * dD, -dBc + y2 * dD, dA + x2 * dD
    return A * dN + 2 * dx2 * x + dxy * y, Bc * dN + 2 * dy2 * y + dxy * x


def mobius_scalar_mul_bwd(r, x, go):
    """(dL/dr per row, dL/dx)."""
    raw = _norm(x)
    n = raw.clamp_min(EPS)
    a = _artanh(n)
    arg = r * a
    t = _tanh(arg)
    tp = _tanh_prime(arg, t)
    gs = _dot(go, x)
    c = _where(raw >= EPS, gs * (tp * r * _artanh_prime(n) * n - t) / (n * n * n))
    return gs * tp * a / n, t / n * go + c * x


def expmap_bwd(x, u, go):
    raw, x2 = _norm(u), _dot(x, x)
    n = raw.clamp_min(EPS)
    c, cp = _conformal(x2)
    arg = n / c
    t = _tanh(arg)
    tp = _tanh_prime(arg, t)
    f = t / n
    dx, ds = mobius_add_bwd(x, f * u, go)
    gf = _dot(ds, u)
    du = f * ds + _where(raw >= EPS, gf * (tp * arg - t) / (n * n * n)) * u
    return dx - 2 * gf * tp / (c * c) * cp * x, du


def logmap_bwd(x, y, go):
    w = mobius_add_ref(-x, y)
    raw, x2 = _norm(w), _dot(x, x)
    n = raw.clamp_min(EPS)
    c, cp = _conformal(x2)
    a = _artanh(n)
    gf = _dot(go, w)
    dw = a * c / n * go + _where(raw >= EPS, gf * c * (_artanh_prime(n) * n - a) / (n * n * n)) * w
    dnx, dy = mobius_add_bwd(-x, y, dw)
    return 2 * gf * a / n * cp * x - dnx, dy


def geodesic_bwd(t, x, y, go):
    """(dL/dt per row, dL/dx, dL/dy)."""
    v = mobius_add_ref(-x, y)
    dx, dtv = mobius_add_bwd(x, mobius_scalar_mul_ref(t, v), go)
    gt, dv = mobius_scalar_mul_bwd(t, v, dtv)
    dnx, dy = mobius_add_bwd(-x, y, dv)
    return gt, dx - dnx, dy


def gyration_bwd(a, b, u, go):
    a2, b2, ab, au, bu = _dot(a, a), _dot(b, b), _dot(a, b), _dot(a, u), _dot(b, u)
    draw = 1 + 2 * ab + a2 * b2
    q = 2 / draw.clamp_min(EPS)
    A, B = -au * b2 + bu + 2 * ab * bu, -bu * a2 - au
    gA, gB = q * _dot(go, a), q * _dot(go, b)
    gd = _where(draw >= EPS, -0.5 * q * (A * gA + B * gB))
    gau, gbu, gab = -b2 * gA - gB, (1 + 2 * ab) * gA - a2 * gB, 2 * (bu * gA + gd)
    ga2, gb2 = -bu * gB + b2 * gd, -au * gA + a2 * gd
    return (q * A * go + gau * u + gab * b + 2 * ga2 * a, q * B * go + gbu * u + gab * a + 2 * gb2 * b, go + gau * a + gbu * b)


def parallel_transport_bwd(x, y, v, go):
    x2, y2 = _dot(x, x), _dot(y, y)
    (cx, cxp), (cy, cyp) = _conformal(x2), _conformal(y2)
    s = cy / cx
    gs = _dot(go, gyration_ref(y, -x, v))
    dy, dnx, dv = gyration_bwd(y, -x, v, s * go)
    return -2 * gs * s / cx * cxp * x - dnx, dy + 2 * gs / cx * cyp * y, dv


def parallel_transport0_bwd(y, v, go):
    c, cp = _conformal(_dot(y, y))
    return 2 * _dot(go, v) * cp * y, c * go


def parallel_transport0back_bwd(x, v, go):
    c, cp = _conformal(_dot(x, x))
    return -2 * _dot(go, v) / (c * c) * cp * x, go / c
