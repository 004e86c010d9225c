"""The yardstick of tests/test_gpu_lstm_seq.py: one bidirectional LSTM layer over T steps as a plain time loop in torch, in the dtype
of its arguments (the GPU tests run it on the CPU in fp64 and in fp32).  tests/test_lstm_seq_reference.py pins it to
``torch.nn.LSTM(...).double()``, forward and every gradient, without a GPU.

The loop keeps what nn.LSTM hides: the gate activations and cell state of every (step, row, direction) in the layout of the kernels'
``saved`` buffer ([i | f | g | o | c], 5 H floats), the hidden state that entered every step, and the pre-activations as explicit
intermediates with ``retain_grad`` -- their gradients are the summands of the parameter gradients, which the reduction rule needs.
"""
import torch

PARAM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
               "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def lstm_seq(x, params, h0=None, c0=None):
    """x (T, rows, K); params: the eight tensors of PARAM_NAMES; h0 / c0 (2, rows, H) or None (zeros).  Returns a dict:
    out (T, rows, 2H), hn, cn (2, rows, H), saved (T, rows, 2, 5, H), pre[d][t] (rows, 4H) in gate order i, f, g, o (graph
    intermediates; retain_grad where a gradient can reach them), hprev[d] (T, rows, H) detached."""
    T, rows, _ = x.shape
    H = params[1].shape[1]
    hs, sv, pre, hprev = [[None] * T, [None] * T], [[None] * T, [None] * T], [[None] * T, [None] * T], [[None] * T, [None] * T]
    hn, cn = [], []
    for d in range(2):
        w_ih, w_hh, b_ih, b_hh = params[4 * d:4 * d + 4]
        h = x.new_zeros(rows, H) if h0 is None else h0[d]
        c = x.new_zeros(rows, H) if c0 is None else c0[d]
        for t in (range(T) if d == 0 else range(T - 1, -1, -1)):
            hprev[d][t] = h.detach()
            a = x[t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
            if a.requires_grad:
                a.retain_grad()
            pre[d][t] = a
            i, f, g, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.tanh(a[:, 2 * H:3 * H]), torch.sigmoid(a[:, 3 * H:])
            c = f * c + i * g
            h = o * torch.tanh(c)
            hs[d][t] = h
            sv[d][t] = torch.stack([i, f, g, o, c], 1)                       # (rows, 5, H)
        hn.append(h)
        cn.append(c)
    out = torch.stack([torch.cat([hs[0][t], hs[1][t]], 1) for t in range(T)])
    saved = torch.stack([torch.stack([sv[0][t], sv[1][t]], 1) for t in range(T)])
    return dict(out=out, hn=torch.stack(hn), cn=torch.stack(cn), saved=saved.detach(), pre=pre,
                hprev=[torch.stack(hprev[0]), torch.stack(hprev[1])])


def run(x, params, h0, c0, g_out=None, g_hn=None, g_cn=None, dtype=torch.float64):
    """Forward and backward of the loop in ``dtype`` from float32 (or any) inputs.  The loss is <out, g_out> + <hn, g_hn> + <cn, g_cn>
    over the upstream gradients that are given.  Returns detached tensors: out, hn, cn, saved, hprev[2]; and, if any upstream gradient
    is given, gx, gh0, gc0 (None without the state), gp (the eight parameter gradients) and dpre[2] (T, rows, 4H)."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)          # hundreds of tiny operations: the thread pool's hand-over costs ten times the arithmetic
    try:
        return _run(x, params, h0, c0, g_out, g_hn, g_cn, dtype)
    finally:
        torch.set_num_threads(threads)


def _run(x, params, h0, c0, g_out, g_hn, g_cn, dtype):
    leaf = lambda t: None if t is None else t.detach().to(dtype).clone().requires_grad_(True)
    xx, hh, cc = leaf(x), leaf(h0), leaf(c0)
    pp = [leaf(p) for p in params]
    r = lstm_seq(xx, pp, hh, cc)
    res = dict(out=r["out"].detach(), hn=r["hn"].detach(), cn=r["cn"].detach(), saved=r["saved"], hprev=r["hprev"])
    ups = [(r[k], g) for k, g in (("out", g_out), ("hn", g_hn), ("cn", g_cn)) if g is not None]
    if not ups:
        return res
    loss = sum((o * g.to(dtype)).sum() for o, g in ups)
    loss.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    res.update(gx=zero(xx), gh0=None if hh is None else zero(hh), gc0=None if cc is None else zero(cc), gp=[zero(p) for p in pp],
               dpre=[torch.stack([zero(a) for a in r["pre"][d]]) for d in range(2)])
    return res
