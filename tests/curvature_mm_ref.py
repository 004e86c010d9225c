"""Plain-torch restatement of dist_matmul, weighted_midpoint_bmm, weighted_midpoint and hyperbolic attention on the Poincare ball at any
negative curvature k = -c, for any dtype: the yardstick of tests/test_gpu_ball_curvature_mm.py, which
tests/test_ball_curvature_mm_host.py holds to the reference's own recorded outputs (tests/golden/curvature_mm.npz) and, at k = -1, to
dist_ref, midpoint_ref and attention_ref.

Written from the formulas of math_.py with its k, clamp by clamp, s = sqrt(-k):
    artan_k(x) = artanh(clamp(s x, +-(1 - 1e-7))) / s        tan_k(x) = tanh(clamp(s x, +-15)) / s                 :218-262, :51-59
    dist_matmul: num = x2 - 2 xy + y2, den = max(1 + 2 k xy + k^2 x2 y2, 1e-15), 2 artan_k(sqrt(max(num / den, 1e-15)))   :937-947
    gamma = 2 / max(1 + k |x|^2, 1e-15)                                                                             :382-383
    mobius_scalar_mul(r, x) = tan_k(r artan_k(n)) x / n, n = max(|x|, 1e-15)                                        :853-858
    project: rows beyond (1 - eps) / s scaled back onto it, eps = 4e-3 (the fp32 eps in every dtype)                :340-352
    midpoints: t = nom / den', a = t / (1 + sqrt(1 + k |t|^2)), den' = max(den, 1e-10) (bmm), clamp_abs(den, 1e-10) (reduce)   :2041-2122
The floors 1e-15 sit on the unscaled ratio and lengths: these are not everywhere the k = -1 functions on operands times s.  Attention is
the composition, with attention_ref's one definition of its own: a query without a finite score has the weights 0.
"""
import math

import torch

EPS, DEN_EPS, BALL_EPS = 1e-15, 1e-10, 4e-3


def _s(k):
    return math.sqrt(-float(k))


def _artan_k(x, k):
    s = _s(k)
    z = (x * s).clamp(-1 + 1e-7, 1 - 1e-7)
    return 0.5 * (torch.log(1 + z) - torch.log(1 - z)) / s


def _tan_k(x, k):
    s = _s(k)
    return (x * s).clamp(-15, 15).tanh() / s


def dist_matmul_ref(x, y, k):
    """x (..., N, D), y (..., D, M) -> (..., N, M)."""
    k = float(k)
    x2 = x.pow(2).sum(dim=-1, keepdim=True)
    y2 = y.pow(2).sum(dim=-2, keepdim=True)
    xy = torch.matmul(x, y)
    num = x2 - 2 * xy + y2
    den = (1 + 2 * k * xy + k * k * x2 * y2).clamp_min(EPS)
    return 2 * _artan_k((num / den).clamp_min(EPS).sqrt(), k)


def gamma_ref(x, k):
    return 2 / (1 + float(k) * x.pow(2).sum(dim=-1, keepdim=True)).clamp_min(EPS)


def mobius_scalar_mul_ref(r, x, k):
    n = x.norm(dim=-1, keepdim=True, p=2).clamp_min(EPS)
    return _tan_k(r * _artan_k(n, k), k) * (x / n)


def project_ref(x, k, eps=BALL_EPS):
    n = x.norm(dim=-1, keepdim=True, p=2).clamp_min(EPS)
    top = (1 - eps) / _s(k)
    return torch.where(n > top, x / n * top, x)


def _halve(t, k):
    return t / (1 + (1 + float(k) * t.pow(2).sum(dim=-1, keepdim=True)).sqrt())


def weighted_midpoint_bmm_ref(xs, weights, k, lincomb=False):
    """xs (..., M, D), weights (..., N, M) -> (..., N, D)."""
    gamma = gamma_ref(xs, k)
    den = torch.matmul(weights.abs(), gamma - 1)
    nom = torch.matmul(weights, gamma * xs)
    a = _halve(nom / den.clamp_min(DEN_EPS), k)
    if lincomb:
        a = mobius_scalar_mul_ref(weights.abs().sum(dim=-1, keepdim=True), a, k)
    return project_ref(a, k)


def weighted_midpoint_ref(xs, k, weights=None, reducedim=None, keepdim=False, lincomb=False, posweight=False, coadd=False):
    """xs (..., D); weights None, of one element, or broadcastable to xs.shape[:-1]; the points of the dimensions ``reducedim``
    (default: all but the last) become one."""
    nd = xs.dim() - 1
    red = list(range(nd)) if reducedim is None else sorted(a % xs.dim() for a in ([reducedim] if isinstance(reducedim, int) else reducedim))
    gamma = gamma_ref(xs, k)
    w = torch.ones((), dtype=xs.dtype, device=xs.device) if weights is None else weights.unsqueeze(-1)
    if posweight and bool((w < 0).any()):
        xs = torch.where(w < 0, -xs, xs)
        w = w.abs()
    den = ((gamma - 1) * w.abs()).sum(red, keepdim=True)
    nom = (gamma * w * xs).sum(red, keepdim=True)
    sg = torch.sign(torch.sign(den) + 0.5)
    t = nom / (sg * (den.abs() + DEN_EPS))
    a = t if (lincomb or coadd) else _halve(t, k)
    if lincomb:
        if w.numel() == 1:
            alpha = w.clone()
            for d in red:
                alpha = alpha * xs.shape[d]
        else:
            alpha = torch.broadcast_tensors(w, gamma)[0].sum(red, keepdim=True)
        a = mobius_scalar_mul_ref(alpha / 2, a, k)
    if not keepdim:
        for i, d in enumerate(red):
            a = a.squeeze(d - i)
    return a


def attention_weights_ref(q, keys, k, beta=1.0, bias=None):
    """softmax_j(-beta d_k(q_i, keys_j) + bias_ij) (..., N, M), all zero in a row without a finite score."""
    s = -beta * dist_matmul_ref(q, keys.transpose(-1, -2), k)
    if bias is not None:
        s = s + bias.to(s.dtype)
    dead = torch.isneginf(s).all(dim=-1, keepdim=True)
    p = torch.softmax(torch.where(dead, torch.zeros_like(s), s), dim=-1)
    return torch.where(dead, torch.zeros_like(p), p)


def hyperbolic_attention_ref(q, keys, values, k, beta=1.0, bias=None):
    """q (..., N, D), keys (..., M, D), values (..., M, E), bias None or broadcastable to (..., N, M) -> (..., N, E)."""
    return weighted_midpoint_bmm_ref(values, attention_weights_ref(q, keys, k, beta, bias), k)
