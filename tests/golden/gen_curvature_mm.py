#!/usr/bin/env python3
"""Generate tests/golden/curvature_mm.npz by running the REFERENCE's own ``dist_matmul``, ``weighted_midpoint_bmm`` and
``weighted_midpoint`` (math_.py:905-947, :1953-2122, imported through tests/golden/refharness.py) at k = -0.5 and k = -2, in fp32 and
fp64, and hyperbolic attention as their composition

    weighted_midpoint_bmm(values, softmax(-beta dist_matmul(q, keys^T, k) + bias, -1), k, lincomb=False)

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_curvature_mm.py

The operands are those of the k = -1 generators -- gen_dist.inputs() (the ``dm_*`` arrays), gen_weighted_midpoint.inputs() (``bmm_*`` and
``red_*``) and gen_attention.inputs() -- with the POINTS divided by sqrt(c), so that they sit at the same relative radius of the ball of
radius 1 / sqrt(c); weights, bias, beta and every grad_output stay as they are.  Per curvature c the operands are stored under
``c<c>.in.<name>`` and, for every case, the output and the autograd gradient of every operand under the case's fixed grad_output under
``c<c>.<case>.<label>``: ``dm``; ``bmm_<kind>_lincomb<0|1>`` for the three kinds of weights; ``red_<name>`` for every entry of
REDUCE_CASES; ``attn_plain`` and ``attn_bias``.  Arrays only.

``main`` asserts that the reference's fp32 run lies within ``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative
to max(1, max|fp64|), and prints the value per array: a condition on the inputs, and the closest any restatement can be held to the
records.  (Its fp64 run projects at (1 - 1e-5) / sqrt(c), its fp32 run at (1 - 4e-3) / sqrt(c): ``main`` asserts that no projected output
comes near either.)  The archive is written with fixed member time stamps, so a second run reproduces the file bit for bit.
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

from geoopt.manifolds.stereographic import math as ref  # noqa: E402

import gen_attention  # noqa: E402
import gen_dist  # noqa: E402
import gen_weighted_midpoint as gen_mid  # noqa: E402

torch.set_num_threads(1)
OWN_FP32_ERROR = 1e-6
CURVATURES = (0.5, 2.0)
BETA = gen_attention.BETA
POINTS = ("dm_x", "dm_y", "bmm_xs", "red_xs", "q", "keys", "values")      # the operands that live on the ball: divided by sqrt(c)
ATTN_LABELS = gen_attention.LABELS


def inputs(c):
    """{name: fp32 array} at curvature -c."""
    ops = {k: a for k, a in gen_dist.inputs().items() if k.startswith("dm_")}
    ops.update({k: a for k, a in gen_mid.inputs().items() if k.startswith(("bmm_", "red_"))})
    ops.update({("attn_" + k if k in ("bias", "grad_output") else k): a for k, a in gen_attention.inputs().items()})
    s = float(np.sqrt(c))
    return {k: ((a.astype(np.float64) / s).astype(np.float32) if k in POINTS else a) for k, a in ops.items()}


def _leaf(a, dt):
    return None if a is None else torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True)


def _run(fn, operands, go, dt, c):
    """fn on leaves of dtype dt at k = -c: [out, grad of every operand that is not None]."""
    leaves = [_leaf(a, dt) for a in operands]
    o = fn(*leaves, torch.tensor(-c, dtype=dt))
    gs = torch.autograd.grad(o, [t for t in leaves if t is not None], torch.from_numpy(go.astype(np.float64)).to(dt).reshape(o.shape))
    return [o.detach()] + list(gs)


def _attention(with_bias, bias):
    def fn(q, keys, values, k):
        s = -BETA * ref.dist_matmul(q, keys.transpose(-1, -2), k)
        if with_bias:
            s = s + torch.from_numpy(bias.astype(np.float64)).to(q.dtype)
        return ref.weighted_midpoint_bmm(values, torch.softmax(s, -1), k, lincomb=False)
    return fn


def cases(ops):
    """[(case, labels, the reference's function of the leaves and k, operands, grad_output, projected)]."""
    out = [("dm", ("out", "grad_x", "grad_y"), lambda a, b, k: ref.dist_matmul(a, b, k), (ops["dm_x"], ops["dm_y"]), ops["dm_grad_output"], False)]
    for kind in gen_mid.BMM_KINDS:
        for lincomb in (False, True):
            out.append((gen_mid.bmm_name(kind, lincomb), ("out", "grad_xs", "grad_w"),
                        lambda x, w, k, lc=lincomb: ref.weighted_midpoint_bmm(x, w, k, lincomb=lc), (ops["bmm_xs"], ops[f"bmm_w_{kind}"]),
                        ops["bmm_grad_output"], True))
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in gen_mid.REDUCE_CASES.items():
        fn = (lambda x, w, k, a=(reducedim, keepdim, lincomb, posweight, coadd):
              ref.weighted_midpoint(x, k, weights=w, reducedim=a[0], keepdim=a[1], lincomb=a[2], posweight=a[3], coadd=a[4]))
        out.append(("red_" + name, ("out", "grad_xs") + (() if wk is None else ("grad_w",)), fn,
                    (ops["red_xs"], None if wk is None else ops[f"red_w_{wk}"]),
                    ops["red_grad_output_all" if reducedim is None else "red_grad_output_r0"], False))
    for name, with_bias in (("attn_plain", False), ("attn_bias", True)):
        out.append((name, ATTN_LABELS, _attention(with_bias, ops["attn_bias"]), (ops["q"], ops["keys"], ops["values"]), ops["attn_grad_output"], True))
    return out


def records(out, c):
    """The inputs and the recorded arrays of every case at curvature -c added to ``out``; returns {array name: the reference's fp32 run
    against its fp64 run}."""
    ops = inputs(c)
    for k, a in ops.items():
        out[f"c{c:g}.in.{k}"] = a
    worst = {}
    for name, labels, fn, operands, go, projected in cases(ops):
        r32, r64 = _run(fn, operands, go, torch.float32, c), _run(fn, operands, go, torch.float64, c)
        if projected:
            assert float(r64[0].norm(dim=-1).max()) * np.sqrt(c) < 0.99, (name, "an output reaches project's sphere")
        for lab, a32, a64 in zip(labels, r32, r64):
            assert bool(torch.isfinite(a32).all()) and bool(torch.isfinite(a64).all()), (name, lab)
            worst[f"c{c:g}.{name}.{lab}"] = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            out[f"c{c:g}.{name}.{lab}"] = a32.numpy()
    return worst


def main():
    out, worst = {}, {}
    for c in CURVATURES:
        worst.update(records(out, c))
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")
    for name, own in worst.items():
        assert own <= OWN_FP32_ERROR, (name, own)
    assert all(a.dtype == np.float32 for a in out.values())
    gen_dist.write_npz(os.path.join(HERE, "curvature_mm.npz"), out)
    w = max(worst, key=worst.get)
    print("curvature_mm.npz written --", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for grp in ("dm", "bmm", "red", "attn"):
        print(" ", grp, f"{max(v for k, v in worst.items() if '.' + grp in k):.2e}")


if __name__ == "__main__":
    main()
