"""Plain-torch restatement of the Moebius GRU (reference: hyperspace/hyrnn_nets.py:61-151, math_.py:1361-1371) at k = -1, in the dtype
of its arguments, written from the formulas:

    T(W, h, U, x, b) = ((W (x) h) (+) (U (x) x)) (+) b
    z = sigmoid(logmap0(T(W_hz, h, W_iz, x, b_z)))      r = sigmoid(logmap0(T(W_hr, h, W_ir, x, b_r)))
    rh = r (.) h      h~ = T(W_hh, rh, W_ih, x, b_h) [expmap0(f(logmap0(.)))]      out = h (+) (z (.) ((-h) (+) h~))

with M (x) v = tanh(|Mv| / |v| artanh |v|) Mv / |Mv| (zero where Mv == 0) and w (.) v the same scaling of w * v (zero where every
|w_e v_e| <= 1e-8); the chunk order of the weights and of the bias is r, h, z.  tests/test_mobius_gru_host.py pins it to the reference's
recorded outputs; tests/test_gpu_mobius_gru.py compares the kernels with it.

``gru_loop_ref`` also returns, per step, the nodes the kernels' reductions run over -- the six products, rh, h_{t-1} and the bias
expanded to one row per input row -- so that the gradients of exactly those nodes are available to the reduction rule.
"""
import torch

from oracle import gmath as og

NONLINS = {"none": None, "tanh": torch.tanh, "relu": torch.relu}


def _scaled(m, v, zero):
    vn = v.norm(dim=-1, keepdim=True, p=2).clamp_min(og.MIN_NORM)
    mn = m.norm(dim=-1, keepdim=True, p=2).clamp_min(og.MIN_NORM)
    res = og.tanh_clamped(mn / vn * og.artanh(vn)) * (m / mn)
    return torch.where(zero, res.new_zeros(()), res)


def matvec_scaled(mv, v):
    """M (x) v given the product mv = v M^T."""
    return _scaled(mv, v, (mv == 0).all(dim=-1, keepdim=True))


def pointwise_mul_ref(w, x):
    wx = w * x
    return _scaled(wx, x, (wx.abs() <= 1e-8).all(dim=-1, keepdim=True))


def transform(mh, h, mx, x, b):
    return og.mobius_add(og.mobius_add(matvec_scaled(mh, h), matvec_scaled(mx, x)), b)


def gru_cell_parts(x, h, w_ih, w_hh, bias, nonlin=None):
    """One step.  bias: (3, H), or (3, rows, H) -- one copy per row.  Returns (out, parts)."""
    H = h.shape[-1]
    b_r, b_h, b_z = bias[0], bias[1], bias[2]
    mx = x @ w_ih.t()
    mhr, mhz = h @ w_hh[:H].t(), h @ w_hh[2 * H:].t()
    z = torch.sigmoid(og.logmap0(transform(mhz, h, mx[:, 2 * H:], x, b_z)))
    r = torch.sigmoid(og.logmap0(transform(mhr, h, mx[:, :H], x, b_r)))
    rh = pointwise_mul_ref(r, h)
    mrh = rh @ w_hh[H:2 * H].t()
    ht = transform(mrh, rh, mx[:, H:2 * H], x, b_h)
    if nonlin is not None:
        ht = og.expmap0(nonlin(og.logmap0(ht)))
    out = og.mobius_add(h, pointwise_mul_ref(z, og.mobius_add(-h, ht)))
    return out, dict(mx=mx, mhr=mhr, mhz=mhz, mrh=mrh, rh=rh, hprev=h, x=x, bias=bias)


def gru_cell_ref(x, h, w_ih, w_hh, bias, nonlin=None):
    return gru_cell_parts(x, h, w_ih, w_hh, bias, nonlin)[0]


def _bias_rows(bias, rows):
    return bias.detach().unsqueeze(1).expand(3, rows, -1).clone().requires_grad_(True)


def gru_loop_ref(x, h0, w_ih, w_hh, bias, nonlin=None, hyperbolic_input=True, hyperbolic_hidden_state0=True, bias_rows=False):
    """x (T, rows, I).  Returns (outs (T, rows, H), h_last, [parts per step]).  bias_rows: every step gets its own (3, rows, H) leaf
    copy of the bias (in parts["bias"]), whose gradients are the per-row bias gradients."""
    h = h0 if hyperbolic_hidden_state0 else og.expmap0(h0)
    if not hyperbolic_input:
        x = og.expmap0(x)
    outs, parts = [], []
    for t in range(x.shape[0]):
        b = _bias_rows(bias, x.shape[1]) if bias_rows else bias
        h, p = gru_cell_parts(x[t], h, w_ih, w_hh, b, nonlin)
        outs.append(h)
        parts.append(p)
    return torch.stack(outs), h, parts


def gru_packed_ref(x, h0, w_ih, w_hh, bias, batch_sizes, nonlin=None, hyperbolic_input=True, hyperbolic_hidden_state0=True, bias_rows=False):
    """Packed sequences: x (sum(batch_sizes), I), step t owns the next batch_sizes[t] rows and the first batch_sizes[t] hidden rows.
    Returns (outs (sum(batch_sizes), H), h_last (batch_sizes[0], H): every row's last state, in the rows' order, [parts per step])."""
    h = h0 if hyperbolic_hidden_state0 else og.expmap0(h0)
    if not hyperbolic_input:
        x = og.expmap0(x)
    outs, done, parts, at = [], [], [], 0
    sizes = [int(b) for b in batch_sizes]
    for t, n in enumerate(sizes):
        h, p = gru_cell_parts(x[at:at + n], h, w_ih, w_hh, _bias_rows(bias, n) if bias_rows else bias, nonlin)
        at += n
        outs.append(h)
        parts.append(p)
        keep = sizes[t + 1] if t + 1 < len(sizes) else 0
        done.insert(0, h[keep:])
        h = h[:keep]
    return torch.cat(outs), torch.cat(done), parts
