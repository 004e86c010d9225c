"""Plain-torch restatement of the geodesic distances on the Poincare ball at k = -1 (math_.py:861-975), for any dtype: the yardstick
of tests/test_gpu_dist.py, which tests/test_dist_host.py holds to the reference's own recorded outputs (tests/golden/dist.npz).

Written from the formulas, clamp by clamp:
    artanh clamps its argument to +-(1 - 1e-7)                                                      :57-59
    mobius_add(x, y) = ((1 + 2 xy + y2) x + (1 - x2) y) / max(1 + 2 xy + x2 y2, 1e-15)              :536-555
    dist(x, y) = 2 artanh(|(-x) (+) y|), dist0(x) = 2 artanh(|x|): the norm without a clamp         :893-902, :973-975
    dist_matmul: num = x2 - 2 xy + y2, den = max(1 - 2 xy + x2 y2, 1e-15), 2 artanh(sqrt(max(num / den, 1e-15)))   :937-947
"""
import torch

EPS = 1e-15


def _artanh(x):
    x = x.clamp(-1 + 1e-7, 1 - 1e-7)
    return 0.5 * (torch.log(1 + x) - torch.log(1 - x))


def mobius_add_ref(x, y):
    x2 = x.pow(2).sum(dim=-1, keepdim=True)
    y2 = y.pow(2).sum(dim=-1, keepdim=True)
    xy = (x * y).sum(dim=-1, keepdim=True)
    return ((1 + 2 * xy + y2) * x + (1 - x2) * y) / (1 + 2 * xy + x2 * y2).clamp_min(EPS)


def dist_ref(x, y, keepdim=False):
    return 2 * _artanh(mobius_add_ref(-x, y).norm(dim=-1, p=2, keepdim=keepdim))


def dist0_ref(x, keepdim=False):
    return 2 * _artanh(x.norm(dim=-1, p=2, keepdim=keepdim))


def dist_matmul_ref(x, y):
    """x (..., N, D), y (..., D, M) -> (..., N, M)."""
    x2 = x.pow(2).sum(dim=-1, keepdim=True)
    y2 = y.pow(2).sum(dim=-2, keepdim=True)
    xy = torch.matmul(x, y)
    num = x2 - 2 * xy + y2
    den = (1 - 2 * xy + x2 * y2).clamp_min(EPS)
    return 2 * _artanh((num / den).clamp_min(EPS).sqrt())
