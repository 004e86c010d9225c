#!/usr/bin/env python3
"""Generate tests/golden/gyro_ops.npz by running the REFERENCE's own ``mobius_sub``, ``mobius_coadd``, ``mobius_cosub``, ``geodesic_unit``,
``lambda_x``, ``inner``, ``norm``, ``egrad2rgrad``, ``sproj`` and ``inv_sproj`` (math_.py:558-589, :678-744, :747-779, :1139-1185, :355-383,
:386-430, :433-472, :1816-1845, :1848-1874, :1877-1905, imported through tests/golden/refharness.py) in fp32 and fp64 at k = -1.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_gyro_ops.py

Operands (10, 5): points x and y within radius 0.8, tangents u and v with norms in [0.1, 1.5], t (10, 1) in [0.1, 3].  The named rows:
x row 1 and y row 2 all zero, x row 3 and y row 4 at norm 0.9, row 5 with x == y, u row 6 all zero, t rows 7, 8, 9 at 0, -1 and 40 -- the
tanh clamp of geodesic_unit holds at t / 2 = 20 and its output lies on the unit sphere.  h (10, 6), the operand of sproj, is inv_sproj of y
computed in fp64.

The calls: mobius_sub(x, y), mobius_coadd(x, y), mobius_cosub(x, y), geodesic_unit(t, x, u), lambda_x(x), inner(x, u, v, keepdim=True),
norm(x, u), egrad2rgrad(x, v), sproj(h), inv_sproj(x).  inner is recorded with keepdim=True: with keepdim=False the reference broadcasts
the rows against each other, (10, 10) here, where the library returns one value per row (hyperspace/gmath.inner).  For every call the
output and the autograd gradients of every operand under one fixed grad_output are recorded, arrays only: grad_output (10, 5) for a
result of that shape, its first column for a result of one value per row, grad_output_wide (10, 6) for inv_sproj.  ``main`` asserts that
the reference's fp32 run lies within ``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative to
max(1, max|fp64|), and prints the value per array.  The archive is written with fixed member time stamps, so a second run reproduces the
file bit for bit.
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

from gen_tangent_maps import _directions, write_npz  # noqa: E402

torch.set_num_threads(1)
SEED = 0
OWN_FP32_ERROR = 1e-6
ROWS, D = 10, 5
ROW_ZERO_X, ROW_ZERO_Y, ROW_RIM_X, ROW_RIM_Y, ROW_SAME, ROW_ZERO_U, ROW_T0, ROW_TNEG, ROW_TBIG = 1, 2, 3, 4, 5, 6, 7, 8, 9
T_NEG, T_BIG = -1.0, 40.0

# name: (labels, the reference's function of the leaves and k, operand keys, grad_output key)
CASES = {
    "mobius_sub": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.mobius_sub(x, y, k=k), ("x", "y"), "grad_output"),
    "mobius_coadd": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.mobius_coadd(x, y, k=k), ("x", "y"), "grad_output"),
    "mobius_cosub": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.mobius_cosub(x, y, k=k), ("x", "y"), "grad_output"),
    "geodesic_unit": (("out", "grad_t", "grad_x", "grad_u"), lambda t, x, u, k: ref.geodesic_unit(t, x, u, k=k), ("t", "x", "u"), "grad_output"),
    "lambda_x": (("out", "grad_x"), lambda x, k: ref.lambda_x(x, k=k), ("x",), "grad_output"),
    "inner": (("out", "grad_x", "grad_u", "grad_v"), lambda x, u, v, k: ref.inner(x, u, v, k=k, keepdim=True), ("x", "u", "v"), "grad_output"),
    "norm": (("out", "grad_x", "grad_u"), lambda x, u, k: ref.norm(x, u, k=k), ("x", "u"), "grad_output"),
    "egrad2rgrad": (("out", "grad_x", "grad_grad"), lambda x, g, k: ref.egrad2rgrad(x, g, k=k), ("x", "v"), "grad_output"),
    "sproj": (("out", "grad_h"), lambda h, k: ref.sproj(h, k=k), ("h",), "grad_output"),
    "inv_sproj": (("out", "grad_x"), lambda x, k: ref.inv_sproj(x, k=k), ("x",), "grad_output_wide"),
}


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    x = _directions(rng, (ROWS, D)) * rng.uniform(0.05, 0.8, (ROWS, 1))
    y = _directions(rng, (ROWS, D)) * rng.uniform(0.05, 0.8, (ROWS, 1))
    u = _directions(rng, (ROWS, D)) * rng.uniform(0.1, 1.5, (ROWS, 1))
    v = _directions(rng, (ROWS, D)) * rng.uniform(0.1, 1.5, (ROWS, 1))
    t = rng.uniform(0.1, 3.0, (ROWS, 1))
    x[ROW_ZERO_X] = 0.0
    y[ROW_ZERO_Y] = 0.0
    x[ROW_RIM_X] *= 0.9 / np.linalg.norm(x[ROW_RIM_X])
    y[ROW_RIM_Y] *= 0.9 / np.linalg.norm(y[ROW_RIM_Y])
    y[ROW_SAME] = x[ROW_SAME]
    u[ROW_ZERO_U] = 0.0
    t[ROW_T0], t[ROW_TNEG], t[ROW_TBIG] = 0.0, T_NEG, T_BIG
    out = dict(x=x, y=y, u=u, v=v, t=t, grad_output=rng.standard_normal((ROWS, D)) / (ROWS * D),
               grad_output_wide=rng.standard_normal((ROWS, D + 1)) / (ROWS * D))
    out = {k: a.astype(np.float32) for k, a in out.items()}
    y64 = torch.from_numpy(out["y"].astype(np.float64))
    out["h"] = ref.inv_sproj(y64, k=torch.tensor(-1.0, dtype=torch.float64)).numpy().astype(np.float32)
    return out


def _grad_output(go, shape):
    """The fixed grad_output for a result of `shape`: itself, or its first column for one value per row."""
    return go.reshape(shape) if go.size == int(np.prod(shape)) else go[:, 0].reshape(shape)


def _run(fn, operands, go, dt):
    leaves = [torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True) for a in operands]
    o = fn(*leaves, torch.tensor(-1.0, dtype=dt))
    gs = torch.autograd.grad(o, leaves, torch.from_numpy(_grad_output(go, tuple(o.shape)).astype(np.float64)).to(dt))
    return [o.detach()] + list(gs)


def records(out):
    """The recorded arrays of every case added to ``out``; returns {array name: the reference's fp32 run against its fp64 run}."""
    worst = {}
    for name, (labels, fn, keys, gk) in CASES.items():
        ops = [out[k] for k in keys]
        r32, r64 = _run(fn, ops, out[gk], torch.float32), _run(fn, ops, out[gk], torch.float64)
        for lab, a32, a64 in zip(labels, r32, r64):
            worst[f"{name}.{lab}"] = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            out[f"{name}.{lab}"] = a32.numpy()
    return worst


def main():
    out = inputs()
    worst = records(out)
    for name, own in worst.items():
        assert own <= OWN_FP32_ERROR, (name, own)
    on_sphere = float(np.linalg.norm(out["geodesic_unit.out"][ROW_TBIG].astype(np.float64)))
    assert abs(on_sphere - 1.0) <= 1e-6, on_sphere             # the tanh clamp holds: |x (+) s| = 1 for |s| = 1
    assert out["inner.out"].shape == (ROWS, 1) and out["lambda_x.out"].shape == out["norm.out"].shape == (ROWS,)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    write_npz(os.path.join(HERE, "gyro_ops.npz"), out)
    w = max(worst, key=worst.get)
    print("gyro_ops.npz written: seed", SEED, "--", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")


if __name__ == "__main__":
    main()
