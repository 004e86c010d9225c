"""The time-loop reference of tests/test_gpu_lstm_seq.py (tests/lstm_seq_ref.py) against ``torch.nn.LSTM(...).double()``: forward and
every gradient within 1e-12, with and without initial states.  No GPU: the yardstick of the GPU sweep is checked where it is written."""
import pytest
import torch

import lstm_seq_ref as lr

TOL = 1e-12


@pytest.mark.parametrize("T,rows,K,H,with_state", [(5, 7, 9, 33, True), (4, 3, 12, 16, False)])
def test_time_loop_reference_is_nn_lstm_in_fp64(T, rows, K, H, with_state):
    g = torch.Generator().manual_seed(100 * T + H)
    torch.manual_seed(T + H)
    lstm = torch.nn.LSTM(K, H, num_layers=1, bidirectional=True).double()
    x = torch.randn(T, rows, K, generator=g, dtype=torch.float64)
    h0 = 0.5 * torch.randn(2, rows, H, generator=g, dtype=torch.float64) if with_state else None
    c0 = 0.5 * torch.randn(2, rows, H, generator=g, dtype=torch.float64) if with_state else None
    ups = [torch.randn(T, rows, 2 * H, generator=g, dtype=torch.float64), torch.randn(2, rows, H, generator=g, dtype=torch.float64),
           torch.randn(2, rows, H, generator=g, dtype=torch.float64)]
    params = [getattr(lstm, n).detach() for n in lr.PARAM_NAMES]
    got = lr.run(x, params, h0, c0, *ups)

    xr = x.clone().requires_grad_(True)
    hx = tuple(t.clone().requires_grad_(True) for t in (h0, c0)) if with_state else None
    out, (hn, cn) = lstm(xr, hx)
    ((out * ups[0]).sum() + (hn * ups[1]).sum() + (cn * ups[2]).sum()).backward()

    def close(a, b, what):
        assert a.shape == b.shape and a.dtype == torch.float64, what
        assert float((a - b.detach()).abs().max()) <= TOL, what

    close(got["out"], out, "out"); close(got["hn"], hn, "h_n"); close(got["cn"], cn, "c_n")
    close(got["gx"], xr.grad, "grad x")
    if with_state:
        close(got["gh0"], hx[0].grad, "grad h0"); close(got["gc0"], hx[1].grad, "grad c0")
    else:
        assert got["gh0"] is None and got["gc0"] is None
    for n, gp in zip(lr.PARAM_NAMES, got["gp"]):
        close(gp, getattr(lstm, n).grad, "grad " + n)
    # what nn.LSTM does not show: `saved` and the pre-activation gradients are consistent with what it does show
    sv = got["saved"]
    assert sv.shape == (T, rows, 2, 5, H)
    for d in range(2):
        o, c = sv[:, :, d, 3], sv[:, :, d, 4]
        close(o * torch.tanh(c), out[:, :, d * H:(d + 1) * H], "saved o, c -> out")
        last = T - 1 if d == 0 else 0
        close(c[last], cn[d], "saved c -> c_n")
        dpre, hprev = got["dpre"][d], got["hprev"][d]
        close(dpre.sum((0, 1)), getattr(lstm, lr.PARAM_NAMES[4 * d + 2]).grad, "colsum dpre -> grad bias")
        close(torch.einsum("trn,trk->nk", dpre, x), getattr(lstm, lr.PARAM_NAMES[4 * d]).grad, "dpre^T x -> grad weight_ih")
        close(torch.einsum("trn,trk->nk", dpre, hprev), getattr(lstm, lr.PARAM_NAMES[4 * d + 1]).grad, "dpre^T h_prev -> grad weight_hh")


def test_time_loop_reference_omits_the_terms_that_are_not_given():
    """One upstream gradient at a time adds up to all three (the loss is linear in them); h0 alone and c0 alone are the zero state
    for the other."""
    g = torch.Generator().manual_seed(3)
    T, rows, K, H = 3, 4, 5, 6
    torch.manual_seed(3)
    lstm = torch.nn.LSTM(K, H, bidirectional=True).double()
    params = [getattr(lstm, n).detach() for n in lr.PARAM_NAMES]
    x = torch.randn(T, rows, K, generator=g, dtype=torch.float64)
    h0, c0 = (0.5 * torch.randn(2, rows, H, generator=g, dtype=torch.float64) for _ in range(2))
    ups = [torch.randn(T, rows, 2 * H, generator=g, dtype=torch.float64), torch.randn(2, rows, H, generator=g, dtype=torch.float64),
           torch.randn(2, rows, H, generator=g, dtype=torch.float64)]
    full = lr.run(x, params, h0, c0, *ups)
    parts = [lr.run(x, params, h0, c0, *[u if i == k else None for i, u in enumerate(ups)]) for k in range(3)]
    for key in ("gx", "gh0", "gc0"):
        assert float((sum(p[key] for p in parts) - full[key]).abs().max()) <= TOL, key
    for k in range(8):
        assert float((sum(p["gp"][k] for p in parts) - full["gp"][k]).abs().max()) <= TOL, k
    only_h = lr.run(x, params, h0, None, *ups)
    zeros = lr.run(x, params, h0, torch.zeros_like(c0), *ups)
    assert only_h["gc0"] is None and torch.equal(only_h["out"], zeros["out"]) and torch.equal(only_h["gx"], zeros["gx"])
    assert "gx" not in lr.run(x, params, None, None)
