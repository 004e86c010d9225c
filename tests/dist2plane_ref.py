"""dist2plane / MobiusDist2Hyperplane at k = -1 restated in plain torch for any dtype (reference: math_.py:1645-1666 with _mobius_add
:537-555 and arsin_k :266-290; the layer: hyperspace/hyrnn_nets.py:210-245).  tests/test_dist2plane_host.py pins it to the reference's own
recorded outputs (tests/golden/mobius_dist2plane.npz); tests/test_gpu_dist2plane.py uses it in fp64 as the reference and in fp32 as
the yardstick of the GPU kernels, as tests/lstm_seq_ref.py serves the LSTM.

Everything is a function of the two products x P^T and x A^T and of per-row / per-plane scalars:

    px = <p,x>   xa = <x,a>   x2 = |x|^2   p2 = |p|^2   pa = <p,a>   an = |a|
    alpha = 1 - 2 px + x2     beta = 1 - p2     D = max(1 - 2 px + p2 x2, 1e-15)
    s  = (beta xa - alpha pa) / D                                        = <(-p) (+) x, a>
    n2 = max((alpha^2 p2 - 2 alpha beta px + beta^2 x2) / D^2, 1e-15)    = |(-p) (+) x|^2
    d  = asinh(2 s' / clamp_abs((1 - n2) an))       s' = s if signed else |s|;   d an if scaled
"""
import torch

EPS = 1e-15


def clamp_abs(v, eps=EPS):
    """geoopt.utils.clamp_abs: sign'(v) (|v| + eps) with sign'(0) = +1."""
    return torch.sign(torch.sign(v) + 0.5) * (v.abs() + eps)


def dist2plane_parts(x, p, a, signed=False, scaled=False, log_scale=None):
    """dist2plane_ref plus the six (rows, N) quantities it is a function of -- px, xa and x2, p2, pa, an expanded to that shape -- as
    nodes of the graph: their gradients are the per-element coefficients C_px, C_xa, C_x2, C_p2, C_pa, C_an whose contractions
    with x, p, a the backward kernels add up (the summands of grad_p, grad_a and the row sums of grad_x)."""
    px, xa = x @ p.t(), x @ a.t()
    x2 = (x * x).sum(-1, keepdim=True).expand_as(px)
    p2, pa, an = ((p * p).sum(-1).expand_as(px), (p * a).sum(-1).expand_as(px), a.norm(dim=-1).expand_as(px))
    parts = dict(px=px, xa=xa, x2=x2, p2=p2, pa=pa, an=an)
    alpha, beta = 1 - 2 * px + x2, 1 - p2
    D = (1 - 2 * px + p2 * x2).clamp_min(EPS)
    s = (beta * xa - alpha * pa) / D
    n2 = ((alpha * alpha * p2 - 2 * alpha * beta * px + beta * beta * x2) / (D * D)).clamp_min(EPS)
    if not signed:
        s = s.abs()
    d = torch.asinh(2 * s / clamp_abs((1 - n2) * an))
    if scaled:
        d = d * an
    return (d if log_scale is None else d * log_scale.exp()), parts


def dist2plane_ref(x, p, a, signed=False, scaled=False, log_scale=None):
    """x (rows, K) on the ball, p (N, K) points of the ball, a (N, K) normals -> (rows, N); times exp(log_scale) (N) where given."""
    return dist2plane_parts(x, p, a, signed, scaled, log_scale)[0]


def layer_ref(x, point, tangent, scale):
    """MobiusDist2Hyperplane.forward (hyrnn_nets.py:227-237) at k = -1: signed, not scaled, times exp(scale)."""
    return dist2plane_ref(x, point, tangent, signed=True, scaled=False, log_scale=scale)
