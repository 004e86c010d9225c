"""Plain-torch restatement of hyperbolic attention at k = -1, for any dtype: the composition of dist_matmul (math_.py:905-947,
tests/dist_ref.py), a softmax over the keys and weighted_midpoint_bmm without lincomb (math_.py:2090-2122, tests/midpoint_ref.py) -- the
yardstick of tests/test_gpu_attention.py, which tests/test_attention_host.py holds to the reference's own recorded outputs
(tests/golden/attention.npz).

    s_ij = -beta d(q_i, keys_j) + bias_ij      p_i = softmax_j s_ij      out_i = weighted_midpoint_bmm(values, p)_i
One definition of its own: a query whose every s_ij is -inf has the weights 0 (the softmax gives NaN), so its output is the origin and
it adds nothing to any gradient.

``attention_backward_formulas`` restates the backward the kernels run (csrc/attention.hip), from the saved row sums, without autograd.
"""
import torch

from dist_ref import dist_matmul_ref
from midpoint_ref import BALL_EPS, DEN_EPS, GAMMA_EPS, gamma_ref, weighted_midpoint_bmm_ref


def attention_weights_ref(q, keys, beta=1.0, bias=None):
    """softmax_j(-beta d(q_i, keys_j) + bias_ij) (..., N, M), all zero in a row without a finite score."""
    s = -beta * dist_matmul_ref(q, keys.transpose(-1, -2))
    if bias is not None:
        s = s + bias.to(s.dtype)
    dead = torch.isneginf(s).all(dim=-1, keepdim=True)
    p = torch.softmax(torch.where(dead, torch.zeros_like(s), s), dim=-1)
    return torch.where(dead, torch.zeros_like(p), p)


def hyperbolic_attention_ref(q, keys, values, beta=1.0, bias=None):
    """q (..., N, D), keys (..., M, D), values (..., M, E), bias None or broadcastable to (..., N, M) -> (..., N, E)."""
    return weighted_midpoint_bmm_ref(values, attention_weights_ref(q, keys, beta, bias))


def attention_backward_formulas(q, keys, values, go, beta=1.0, bias=None):
    """(grad_q, grad_keys, grad_values) from the formulas of csrc/attention.hip, 3-D operands of one dtype; autograd is used for the two
    row maps alone (the midpoint's tail and the pair distance), whose own backward other tests hold."""
    with torch.enable_grad():
        p = attention_weights_ref(q, keys, beta, bias).detach()
        gamma = gamma_ref(values)                                           # (b, M, 1)
        c = gamma - 1
        nom = torch.matmul(p, gamma * values).requires_grad_(True)
        den = torch.matmul(p, c).requires_grad_(True)
        t = nom / den.clamp_min(DEN_EPS)
        a = t / (1 + (1 - t.pow(2).sum(dim=-1, keepdim=True)).sqrt())
        n = a.norm(dim=-1, keepdim=True, p=2).clamp_min(1e-15)
        out = torch.where(n > 1 - BALL_EPS, a / n * (1 - BALL_EPS), a)
        g_s, g_d = torch.autograd.grad(out, [nom, den], go)
        nom, den = nom.detach(), den.detach()
        delta = (g_s * nom).sum(-1, keepdim=True) + g_d * den              # (b, N, 1)
        gw = torch.matmul(g_s, (gamma * values).transpose(-1, -2)) + g_d * c.transpose(-1, -2)
        gs = p * (gw - delta)
        G = torch.matmul(p.transpose(-1, -2), g_s)
        h = torch.matmul(p.transpose(-1, -2), g_d)
        live = (1 - values.pow(2).sum(dim=-1, keepdim=True)) >= GAMMA_EPS
        grad_v = gamma * G + torch.where(live, gamma * gamma * ((G * values).sum(-1, keepdim=True) + h), torch.zeros_like(h)) * values
        ql, kl = q.detach().clone().requires_grad_(True), keys.detach().clone().requires_grad_(True)
        d = dist_matmul_ref(ql, kl.transpose(-1, -2))
        grad_q, grad_k = torch.autograd.grad(d, [ql, kl], -beta * gs)
    return grad_q, grad_k, grad_v
