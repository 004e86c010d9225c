"""Operand shapes the C ABI cannot see.  The entry points receive pointers and one set of sizes; a wrapper that takes the sizes from one
operand and never looks at the other lets the kernel read past the end of a device buffer.  Every differentiable wrapper therefore compares
its operands' shapes before it asks for a device tensor, and raises an error that names both shapes.

Host tensors only (the pattern of tests/test_dist2plane_host.py): no device call can happen.  Each entry is a pair of calls -- one with
operands that fit, which must get past the shape check and stop at the "must live on the GPU" error, and the mismatched ones, which must
stop at the shape error (``HypadError``; ``NotImplementedError`` where that is the function's convention for what it does not take).
"""
import re
from types import SimpleNamespace

import pytest
import torch

Z = torch.zeros


def _lstm(k, h):
    return torch.nn.LSTM(k, h, bidirectional=True).requires_grad_(False)


def _named(lstm, **replace):
    """The eight tensors of layer 0 as attributes of a plain holder, some replaced."""
    d = {n: p.detach() for n, p in lstm.named_parameters()}
    d.update(replace)
    return SimpleNamespace(parameters=lambda: iter(()), **d)


def _entries():
    from hypad_amd import autograd as hag
    from hypad_amd.hyperspace import gmath, hyrnn_nets
    E, N = "HypadError", "NotImplementedError"
    lin = lambda **kw: (lambda x, w, b: hyrnn_nets.mobius_linear(x, w, b, **kw))
    original = lin(hyperbolic_input=False, hyperbolic_bias=True)                # -> _MobiusLinearFn
    general = lin(hyperbolic_input=True, hyperbolic_bias=False, nonlin=torch.tanh)   # -> _MobiusLinearExFn
    layer = hyrnn_nets.MobiusLinear(8, 5, hyperbolic_input=False, fp64_hyper=False)
    layer_ex = hyrnn_nets.MobiusLinear(8, 5, fp64_hyper=False)
    d2p = hyrnn_nets.MobiusDist2Hyperplane(8, 5)
    lstm = _lstm(6, 4)
    seq = lambda x, holder=lstm, hx=None: hag.lstm_seq(x, holder, 0, hx)

    def fwd(x, holder=lstm, hx=None):
        with torch.no_grad():
            return hag.lstm_seq_forward(x, holder, 0, hx)
    hx = lambda rows=3, h=4, n=2: (Z(n, rows, h), Z(n, rows, h))
    # (name, error type, the call with operands that fit, the mismatched calls)
    out = [
        ("poincare_rowdist", E, lambda: gmath.poincare_rowdist(Z(4, 8), Z(4, 8)),
         [lambda: gmath.poincare_rowdist(Z(4, 8), Z(3, 8)), lambda: gmath.poincare_rowdist(Z(4, 8), Z(1, 8)),
          lambda: gmath.poincare_rowdist(Z(4, 8), Z(4, 7)), lambda: gmath.poincare_rowdist(Z(4, 8), Z(8))]),
        ("hyperbolic_loss", E, lambda: gmath.hyperbolic_loss(Z(4, 8), Z(4, 8), 4),
         [lambda: gmath.hyperbolic_loss(Z(4, 8), Z(3, 8), 4), lambda: gmath.hyperbolic_loss(Z(4, 8), Z(1, 8), 4),
          lambda: gmath.hyperbolic_loss(Z(4, 8), Z(4, 9), 4)]),
        ("mobius_add", E, lambda: gmath.mobius_add(Z(4, 8), Z(4, 8)),
         # (y (4, 8) against x (2, 4, 8) broadcasts, as in the reference: tests/test_layer_call_forms_host.py; (3, 8) does not)
         [lambda: gmath.mobius_add(Z(4, 8), Z(4, 7)), lambda: gmath.mobius_add(Z(4, 8), Z(9)), lambda: gmath.mobius_add(Z(2, 4, 8), Z(3, 8))]),
        ("mobius_add, one row", E, lambda: gmath.mobius_add(Z(4, 8), Z(8)), [lambda: gmath.mobius_add(Z(4, 8), Z(7))]),
        ("mobius_pointwise_mul", N, lambda: gmath.mobius_pointwise_mul(Z(4, 8), Z(4, 8)),
         [lambda: gmath.mobius_pointwise_mul(Z(4, 7), Z(4, 8)), lambda: gmath.mobius_pointwise_mul(Z(9), Z(4, 8)),
          lambda: gmath.mobius_pointwise_mul(Z(3, 8), Z(4, 8))]),
        ("mobius_linear, the original configuration", E, lambda: original(Z(4, 8), Z(5, 8), Z(5)),
         [lambda: original(Z(4, 7), Z(5, 8), Z(5)), lambda: original(Z(4, 8), Z(5, 8), Z(8)), lambda: original(Z(4, 8), Z(5, 8), Z(1, 5))]),
        ("mobius_linear, the general function", E, lambda: general(Z(4, 8), Z(5, 8), Z(5)),
         [lambda: general(Z(4, 9), Z(5, 8), Z(5)), lambda: general(Z(4, 8), Z(5, 8), Z(4)), lambda: general(Z(8, 4), Z(5, 8), None)]),
        ("MobiusLinear", E, lambda: layer(Z(4, 8)), [lambda: layer(Z(4, 5)), lambda: layer(Z(4, 9))]),
        ("MobiusLinear on the ball", E, lambda: layer_ex(Z(4, 8)), [lambda: layer_ex(Z(4, 5))]),
        ("MobiusDist2Hyperplane", E, lambda: d2p(Z(4, 8)), [lambda: d2p(Z(4, 5)), lambda: d2p(Z(4, 9)), lambda: d2p(Z(8, 4))]),
        ("mobius_matvec", E, lambda: gmath.mobius_matvec(Z(5, 8), Z(4, 8)),
         [lambda: gmath.mobius_matvec(Z(5, 8), Z(4, 5)), lambda: hyrnn_nets.mobius_matvec(Z(5, 8), Z(4, 9), k=-1.0)]),
        ("linear_act", E, lambda: hag.linear_act(Z(4, 8), Z(5, 8), Z(5)),
         [lambda: hag.linear_act(Z(4, 7), Z(5, 8), Z(5)), lambda: hag.linear_act(Z(4, 8), Z(5, 8), Z(8)),
          lambda: hag.linear_act(Z(4, 8), Z(5, 8), Z(4)), lambda: hag.linear_act(Z(8), Z(5, 8), Z(5))]),
        ("lstm_layer", E, lambda: hag.lstm_layer(Z(3, 6), lstm, 0),
         [lambda: hag.lstm_layer(Z(3, 5), lstm, 0), lambda: hag.lstm_layer(Z(3, 16), lstm, 0),
          lambda: hag.lstm_layer(Z(3, 6), _named(lstm, weight_ih_l0_reverse=Z(16, 7)), 0)]),
        ("lstm_seq", E, lambda: seq(Z(2, 3, 6)), [lambda: seq(Z(2, 3, 7)), lambda: seq(Z(3, 6))]),
        ("lstm_seq with states", E, lambda: seq(Z(2, 3, 6), hx=hx()),
         [lambda: seq(Z(2, 3, 6), hx=hx(rows=2)), lambda: seq(Z(2, 3, 6), hx=hx(h=5)), lambda: seq(Z(2, 3, 6), hx=hx(n=1)),
          lambda: seq(Z(2, 3, 6), hx=(Z(2, 3, 4), Z(2, 4, 4))), lambda: seq(Z(2, 3, 6), hx=(Z(3, 4), Z(2, 3, 4)))]),
        ("lstm_seq_forward", E, lambda: fwd(Z(2, 3, 6)), [lambda: fwd(Z(2, 3, 5)), lambda: fwd(Z(2, 3, 6), _named(lstm, weight_hh_l0=Z(16, 5)))]),
        ("lstm_seq_forward with states", E, lambda: fwd(Z(2, 3, 6), hx=hx()),
         [lambda: fwd(Z(2, 3, 6), hx=hx(rows=4)), lambda: fwd(Z(2, 3, 6), hx=hx(h=3)), lambda: fwd(Z(2, 3, 6), hx=(Z(2, 3, 4), Z(1, 3, 4)))]),
    ]
    return out


NAMES = ["poincare_rowdist", "hyperbolic_loss", "mobius_add", "mobius_add, one row", "mobius_pointwise_mul",
         "mobius_linear, the original configuration", "mobius_linear, the general function", "MobiusLinear", "MobiusLinear on the ball",
         "MobiusDist2Hyperplane", "mobius_matvec", "linear_act", "lstm_layer", "lstm_seq", "lstm_seq with states", "lstm_seq_forward",
         "lstm_seq_forward with states"]
SHAPE = re.compile(r"\(\d*,?( ?\d+,?)*\)")            # a printed shape: (4, 8), (8,), ()


def test_the_table_names_every_wrapper():
    assert [e[0] for e in _entries()] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_mismatched_operands_are_refused_before_any_device_tensor(name):
    from hypad_amd import _C
    _, kind, fits, mismatched = next(e for e in _entries() if e[0] == name)
    # operands that fit get past the shape check and stop where a device tensor is asked for: the check does not refuse everything
    with pytest.raises(_C.HypadError, match="must live on the GPU"):
        fits()
    err = _C.HypadError if kind == "HypadError" else NotImplementedError
    for i, call in enumerate(mismatched):
        with pytest.raises(err) as info:
            call()
        msg = str(info.value)
        assert "must live on the GPU" not in msg, (name, i, msg)
        assert len(SHAPE.findall(msg)) >= 2, f"{name}, call {i}: the error does not name both shapes: {msg}"
