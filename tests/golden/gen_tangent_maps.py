#!/usr/bin/env python3
"""Generate tests/golden/tangent_maps.npz by running the REFERENCE's own ``expmap``, ``logmap``, ``geodesic``, ``gyration``,
``parallel_transport``, ``parallel_transport0`` and ``parallel_transport0back`` (math_.py:1052-1102, :1188-1230, :978-1049, :592-675,
:1669-1746, :1749-1779, :1782-1813, imported through tests/golden/refharness.py) in fp32 and fp64 at k = -1.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_tangent_maps.py

Operands (10, 5): points x and y within radius 0.8, a tangent u with norms in [0.1, 1.5], t (10, 1) in [0.1, 0.9].  The named rows:
x row 1 and y row 2 all zero, x row 3 and y row 4 at norm 0.9, u row 5 all zero, u row 6 at norm 12 with x row 6 at norm 0.6 -- the tanh clamp of
expmap holds there and its output lies on the unit sphere --, t rows 7, 8, 9 at 0, 1 and -0.25.  No row has x == y: there the reference's fp32
artanh, a difference of two logarithms, returns gradient 0 where the library follows artanh(n) / n -> 1 (hyperspace/gmath.logmap);
``main`` asserts that no x / y pair is closer than 0.1 in Euclidean distance.  No t beyond [-0.25, 1]: with t up to 1.5 the
reference's own fp32 geodesic leaves its fp64 run by more than the bound below.

The calls: expmap(x, u), logmap(x, y), geodesic(t, x, y), gyration(x, y, u), parallel_transport(x, y, u), parallel_transport0(y, u),
parallel_transport0back(x, u).  For every one the output and the autograd gradients of every operand under one fixed grad_output,
N(0, 1) / out.numel(), are recorded: arrays only.  ``main`` asserts that the reference's fp32 run lies within ``OWN_FP32_ERROR`` = 1e-6
of its own fp64 run on every recorded array, relative to max(1, max|fp64|), and prints the worst value per array.  The seed is one
that passes both assertions (docs/history/tangent_maps.md lists the ones tried).  The archive is written with fixed member time
stamps, so a second run reproduces the file bit for bit.
"""
import io
import os
import sys
import zipfile

os.environ.setdefault("PYTORCH_JIT", "0")
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import refharness  # noqa: E402

refharness.install()

from geoopt.manifolds.stereographic import math as ref  # noqa: E402

torch.set_num_threads(1)
SEED = 3
OWN_FP32_ERROR = 1e-6
ROWS, D = 10, 5
ROW_ZERO_X, ROW_ZERO_Y, ROW_RIM_X, ROW_RIM_Y, ROW_ZERO_U, ROW_LONG_U, ROW_T0, ROW_T1, ROW_TNEG = 1, 2, 3, 4, 5, 6, 7, 8, 9
LONG_U, T_NEG = 12.0, -0.25
MIN_SEPARATION = 0.1

# name: (labels, the reference's function of the leaves and k, operand keys)
CASES = {
    "expmap": (("out", "grad_x", "grad_u"), lambda x, u, k: ref.expmap(x, u, k=k), ("x", "u")),
    "logmap": (("out", "grad_x", "grad_y"), lambda x, y, k: ref.logmap(x, y, k=k), ("x", "y")),
    "geodesic": (("out", "grad_t", "grad_x", "grad_y"), lambda t, x, y, k: ref.geodesic(t, x, y, k=k), ("t", "x", "y")),
    "gyration": (("out", "grad_a", "grad_b", "grad_u"), lambda a, b, u, k: ref.gyration(a, b, u, k=k), ("x", "y", "u")),
    "parallel_transport": (("out", "grad_x", "grad_y", "grad_v"), lambda x, y, v, k: ref.parallel_transport(x, y, v, k=k), ("x", "y", "u")),
    "parallel_transport0": (("out", "grad_y", "grad_v"), lambda y, v, k: ref.parallel_transport0(y, v, k=k), ("y", "u")),
    "parallel_transport0back": (("out", "grad_x", "grad_v"), lambda x, v, k: ref.parallel_transport0back(x, v, k=k), ("x", "u")),
}


def _directions(rng, shape):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def inputs(seed=SEED):
    rng = np.random.default_rng(seed)
    x = _directions(rng, (ROWS, D)) * rng.uniform(0.05, 0.8, (ROWS, 1))
    y = _directions(rng, (ROWS, D)) * rng.uniform(0.05, 0.8, (ROWS, 1))
    u = _directions(rng, (ROWS, D)) * rng.uniform(0.1, 1.5, (ROWS, 1))
    t = rng.uniform(0.1, 0.9, (ROWS, 1))
    x[ROW_ZERO_X] = 0.0
    y[ROW_ZERO_Y] = 0.0
    x[ROW_RIM_X] *= 0.9 / np.linalg.norm(x[ROW_RIM_X])
    y[ROW_RIM_Y] *= 0.9 / np.linalg.norm(y[ROW_RIM_Y])
    u[ROW_ZERO_U] = 0.0
    u[ROW_LONG_U] *= LONG_U / np.linalg.norm(u[ROW_LONG_U])
    x[ROW_LONG_U] *= 0.6 / np.linalg.norm(x[ROW_LONG_U])    # lambda_x |u| / 2 = 12 / 0.64 = 18.75, above the clamp at 15
    t[ROW_T0], t[ROW_T1], t[ROW_TNEG] = 0.0, 1.0, T_NEG
    out = dict(x=x, y=y, u=u, t=t, grad_output=rng.standard_normal((ROWS, D)) / (ROWS * D))
    return {k: v.astype(np.float32) for k, v in out.items()}


def write_npz(path, arrays):
    """np.savez with the members' time stamps pinned (numpy stamps them with the wall clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def _run(fn, operands, go, dt):
    leaves = [torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True) for a in operands]
    o = fn(*leaves, torch.tensor(-1.0, dtype=dt))
    gs = torch.autograd.grad(o, leaves, torch.from_numpy(go.astype(np.float64)).to(dt).reshape(o.shape))
    return [o.detach()] + list(gs)


def separation(out):
    return float(np.linalg.norm(out["x"].astype(np.float64) - out["y"].astype(np.float64), axis=-1).min())


def records(out):
    """The recorded arrays of every case added to ``out``; returns {array name: the reference's fp32 run against its fp64 run}."""
    worst = {}
    for name, (labels, fn, keys) in CASES.items():
        ops = [out[k] for k in keys]
        r32, r64 = _run(fn, ops, out["grad_output"], torch.float32), _run(fn, ops, out["grad_output"], torch.float64)
        for lab, a32, a64 in zip(labels, r32, r64):
            worst[f"{name}.{lab}"] = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            out[f"{name}.{lab}"] = a32.numpy()
    return worst


def main():
    out = inputs()
    sep = separation(out)
    assert sep >= MIN_SEPARATION, sep
    worst = records(out)
    for name, own in worst.items():
        assert own <= OWN_FP32_ERROR, (name, own)
    on_sphere = float(np.linalg.norm(out["expmap.out"][ROW_LONG_U].astype(np.float64)))
    assert abs(on_sphere - 1.0) <= 1e-6, on_sphere             # the tanh clamp holds: |x (+) s| = 1 for |s| = 1
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in out.values())
    write_npz(os.path.join(HERE, "tangent_maps.npz"), out)
    w = max(worst, key=worst.get)
    print("tangent_maps.npz written: seed", SEED, "--", len(out), "arrays; smallest |x - y|", f"{sep:.3f};",
          "the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")


if __name__ == "__main__":
    main()
