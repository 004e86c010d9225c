"""Plain-torch restatement of the weighted Moebius gyromidpoint in both forms and of mobius_scalar_mul at k = -1
(math_.py:1953-2122, :788-858), for any dtype: the yardstick of tests/test_gpu_weighted_midpoint.py, which
tests/test_weighted_midpoint_host.py holds to the reference's own recorded outputs (tests/golden/weighted_midpoint.npz).

Written from the formulas, clamp by clamp:
    gamma = 2 / max(1 - |x|^2, 1e-15)                                       _lambda_x :382-383
    artanh clamps its argument to +-(1 - 1e-7), tanh to +-15                :51-59
    mobius_scalar_mul(r, x) = tanh(r artanh |x|) x / |x|, |x| >= 1e-15      :853-858
    project: rows beyond 1 - eps scaled back onto it, eps = 4e-3            :340-352 (the fp32 eps in every dtype: the kernels' sphere)
    clamp_abs(d, 1e-10) = sign'(d) (|d| + 1e-10), sign'(0) = +1             geoopt.utils
"""
import torch

GAMMA_EPS, DEN_EPS, MIN_NORM, BALL_EPS = 1e-15, 1e-10, 1e-15, 4e-3


def _artanh(x):
    x = x.clamp(-1 + 1e-7, 1 - 1e-7)
    return 0.5 * (torch.log(1 + x) - torch.log(1 - x))


def _tanh(x):
    return x.clamp(-15, 15).tanh()


def gamma_ref(x):
    return 2 / (1 - x.pow(2).sum(dim=-1, keepdim=True)).clamp_min(GAMMA_EPS)


def mobius_scalar_mul_ref(r, x):
    n = x.norm(dim=-1, keepdim=True, p=2).clamp_min(MIN_NORM)
    return _tanh(r * _artanh(n)) * (x / n)


def project_ref(x, eps=BALL_EPS):
    n = x.norm(dim=-1, keepdim=True, p=2).clamp_min(MIN_NORM)
    return torch.where(n > 1 - eps, x / n * (1 - eps), x)


def _halve(t):
    return t / (1 + (1 - t.pow(2).sum(dim=-1, keepdim=True)).sqrt())


def weighted_midpoint_bmm_ref(xs, weights, lincomb=False, eps=BALL_EPS, parts=None):
    """xs (..., M, D), weights (..., N, M) -> (..., N, D).  parts: a dict that receives the nodes nom, den and alpha."""
    gamma = gamma_ref(xs)
    den = torch.matmul(weights.abs(), gamma - 1)
    nom = torch.matmul(weights, gamma * xs)
    alpha = weights.abs().sum(dim=-1, keepdim=True)
    if parts is not None:
        parts.update(nom=nom, den=den, alpha=alpha)
    a = _halve(nom / den.clamp_min(DEN_EPS))
    if lincomb:
        a = mobius_scalar_mul_ref(alpha, a)
    return project_ref(a, eps)


def weighted_midpoint_ref(xs, weights=None, reducedim=None, keepdim=False, lincomb=False, posweight=False, coadd=False):
    """xs (..., D); weights None, of one element, or broadcastable to xs.shape[:-1]; the points of the dimensions ``reducedim``
    (default: all but the last) become one."""
    nd = xs.dim() - 1
    red = list(range(nd)) if reducedim is None else sorted(a % xs.dim() for a in ([reducedim] if isinstance(reducedim, int) else reducedim))
    gamma = gamma_ref(xs)
    w = torch.ones((), dtype=xs.dtype, device=xs.device) if weights is None else weights.unsqueeze(-1)
    if posweight and bool((w < 0).any()):
        xs = torch.where(w < 0, -xs, xs)
        w = w.abs()
    den = ((gamma - 1) * w.abs()).sum(red, keepdim=True)
    nom = (gamma * w * xs).sum(red, keepdim=True)
    s = torch.sign(torch.sign(den) + 0.5)
    t = nom / (s * (den.abs() + DEN_EPS))
    a = t if (lincomb or coadd) else _halve(t)
    if lincomb:
        if w.numel() == 1:
            alpha = w.clone()
            for d in red:
                alpha = alpha * xs.shape[d]
        else:
            alpha = torch.broadcast_tensors(w, gamma)[0].sum(red, keepdim=True)
        a = mobius_scalar_mul_ref(alpha / 2, a)
    if not keepdim:
        for i, d in enumerate(red):
            a = a.squeeze(d - i)
    return a
