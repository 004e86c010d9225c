#!/usr/bin/env python3
"""Generate tests/golden/curvature.npz by running the REFERENCE's own 25 row-wise functions (math_.py, imported through
tests/golden/refharness.py) at k = -0.5 and k = -2, in fp32 and fp64.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_curvature.py

The operands are those of the k = -1 generators with the POINTS divided by sqrt(c), so that they sit at the same relative radius of the
ball of radius 1 / sqrt(c); tangents, t and r stay as they are.  Per curvature c (keys ``c<c>.<set>.<operand>``):
    set ``tan`` -- gen_tangent_maps.inputs(): x, y, u, t, grad_output (10, 5), separated points, rim rows at 0.9 / sqrt(c) -- for the seven
        tangent maps and for project(x), expmap0(u), mobius_add(x, y), mobius_pointwise_mul(u, x), dist(x, y), dist0(x);
    set ``gyro`` -- gen_gyro_ops.inputs(): x, y, u, v, t, h, grad_output, grad_output_wide with its named rows (x == y among them), h =
        inv_sproj(y) computed in fp64 at that k -- for the ten gyro ops;
    set ``nz`` -- the ``tan`` set without its all-zero point rows (8 rows) -- for logmap0(y) and mobius_scalar_mul(t, x): at an all-zero
        row the reference's fp32 gradient is off by 3e-2 from its own fp64 (its artanh is a difference of two logarithms).
dist does not see an x == y row: there the reference is off by 6e-4 from its own fp64.

For every call the output and the autograd gradients of every operand under the set's fixed grad_output are recorded under
``c<c>.<function>.<label>``, arrays only; inner is recorded with keepdim=True (gen_gyro_ops.py says why).  ``main`` asserts that the
reference's fp32 run lies within ``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative to max(1, max|fp64|),
and prints the value per array.  The archive is written with fixed member time stamps, so a second run reproduces the file bit for bit.
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

import gen_gyro_ops  # noqa: E402
import gen_tangent_maps  # noqa: E402

torch.set_num_threads(1)
OWN_FP32_ERROR = 1e-6
CURVATURES = (0.5, 2.0)
POINTS = ("x", "y")                                            # the operands that live on the ball: divided by sqrt(c)

# name: (labels, the reference's function of the leaves and k, operand set, operand keys, grad_output key)
CASES = {
    "project": (("out", "grad_x"), lambda x, k: ref.project(x, k=k), "tan", ("x",), "grad_output"),
    "expmap0": (("out", "grad_u"), lambda u, k: ref.expmap0(u, k=k), "tan", ("u",), "grad_output"),
    "logmap0": (("out", "grad_y"), lambda y, k: ref.logmap0(y, k=k), "nz", ("y",), "grad_output"),
    "mobius_add": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.mobius_add(x, y, k=k), "tan", ("x", "y"), "grad_output"),
    "mobius_pointwise_mul": (("out", "grad_w", "grad_x"), lambda w, x, k: ref.mobius_pointwise_mul(w, x, k=k), "tan", ("u", "x"), "grad_output"),
    "mobius_scalar_mul": (("out", "grad_r", "grad_x"), lambda r, x, k: ref.mobius_scalar_mul(r, x, k=k), "nz", ("t", "x"), "grad_output"),
    "dist": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.dist(x, y, k=k), "tan", ("x", "y"), "grad_output"),
    "dist0": (("out", "grad_x"), lambda x, k: ref.dist0(x, k=k), "tan", ("x",), "grad_output"),
}
CASES.update({name: (labels, fn, "tan", keys, "grad_output") for name, (labels, fn, keys) in gen_tangent_maps.CASES.items()})
CASES.update({name: (labels, fn, "gyro", keys, gk) for name, (labels, fn, keys, gk) in gen_gyro_ops.CASES.items()})


def inputs(c):
    """{set: {operand: fp32 array}} at curvature -c."""
    s = float(np.sqrt(c))
    tan = {k: a.astype(np.float64) for k, a in gen_tangent_maps.inputs().items()}
    gyro = {k: a.astype(np.float64) for k, a in gen_gyro_ops.inputs().items() if k != "h"}
    for ops in (tan, gyro):
        for p in POINTS:
            ops[p] = ops[p] / s
    tan = {k: a.astype(np.float32) for k, a in tan.items()}
    gyro = {k: a.astype(np.float32) for k, a in gyro.items()}
    y64 = torch.from_numpy(gyro["y"].astype(np.float64))
    gyro["h"] = ref.inv_sproj(y64, k=torch.tensor(-c, dtype=torch.float64)).numpy().astype(np.float32)
    keep = [r for r in range(gen_tangent_maps.ROWS) if r not in (gen_tangent_maps.ROW_ZERO_X, gen_tangent_maps.ROW_ZERO_Y)]
    nz = {k: a[keep] for k, a in tan.items()}
    return dict(tan=tan, gyro=gyro, nz=nz)


def _run(fn, operands, go, dt, c):
    leaves = [torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True) for a in operands]
    o = fn(*leaves, torch.tensor(-c, dtype=dt))
    gs = torch.autograd.grad(o, leaves, torch.from_numpy(gen_gyro_ops._grad_output(go, tuple(o.shape)).astype(np.float64)).to(dt))
    return [o.detach()] + list(gs)


def records(out, c):
    """The inputs and the recorded arrays of every case at curvature -c added to ``out``; returns {array name: the reference's fp32 run
    against its fp64 run}."""
    sets = inputs(c)
    for sname, ops in sets.items():
        for k, a in ops.items():
            out[f"c{c:g}.{sname}.{k}"] = a
    worst = {}
    for name, (labels, fn, sname, keys, gk) in CASES.items():
        ops = [sets[sname][k] for k in keys]
        r32, r64 = _run(fn, ops, sets[sname][gk], torch.float32, c), _run(fn, ops, sets[sname][gk], torch.float64, c)
        for lab, a32, a64 in zip(labels, r32, r64):
            worst[f"c{c:g}.{name}.{lab}"] = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            out[f"c{c:g}.{name}.{lab}"] = a32.numpy()
    return worst


def main():
    assert len(CASES) == 25
    out, worst = {}, {}
    for c in CURVATURES:
        worst.update(records(out, c))
        tan = {k.split(".")[-1]: a for k, a in out.items() if k.startswith(f"c{c:g}.tan.")}
        assert gen_tangent_maps.separation(tan) >= gen_tangent_maps.MIN_SEPARATION / np.sqrt(c)
    for name, own in worst.items():
        assert own <= OWN_FP32_ERROR, (name, own)
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in out.values())
    gen_tangent_maps.write_npz(os.path.join(HERE, "curvature.npz"), out)
    w = max(worst, key=worst.get)
    print("curvature.npz written --", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")


if __name__ == "__main__":
    main()
