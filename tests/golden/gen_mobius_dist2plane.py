#!/usr/bin/env python3
"""Generate tests/golden/mobius_dist2plane.npz by running the REFERENCE's own ``dist2plane`` (math_.py:1599-1666, imported through
tests/golden/refharness.py) in fp32 on one small input.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mobius_dist2plane.py

The function is called as the reference's layer calls it (hyperspace/hyrnn_nets.py:233-236), ``dist2plane(x.unsqueeze(-2), p, a, ...)``,
but with k = -1: the class passes ``k=self.ball.c`` = +1, which today's math_.py reads as the spherical model, and it cannot be
instantiated under the harness (the Sphere stub has no proj_).  Cases: signed x scaled -- four -- plus the layer form, signed and not
scaled times exp(scale).  9 rows, K = 7, N = 5; row 3 is all zero, row 5 has norm 0.9, row 7 equals the point of plane 2.  For every
case the output and the gradients of x, p, a (and scale) under one fixed grad_output are recorded -- arrays only.  The archive is
written with fixed member time stamps, so a second run reproduces the file bit for bit.

grad_output.  tests/test_dist2plane_host.py holds a restatement to these fp32 records at 1e-6 relative to max(1, max|record|), and no
restatement can come closer to them than the reference's fp32 run is to its own fp64 run.  With a row at norm 0.9 (conformal factor
10.5) that distance is 4e-7 .. 1.1e-5 of a gradient's largest entry (seeds 21 .. 32 with grad_output ~ N(0, 1), whose gradients reach
5 .. 16), so the fixed grad_output is that of a mean-reduced loss with N(0, 1) weights, N(0, 1) / (ROWS * N): the gradients stay below
1, the bound is an absolute 1e-6 on them, and ``main`` asserts that the reference's fp32 run lies within 5e-7 of its fp64 run on every
recorded array (for the unsigned forms without the pair (row 7, plane 2): row 7 lies ON plane 2, where |s| has its kink and the sign
of that pair's gradient is rounding noise in any precision).
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

from geoopt.manifolds.stereographic.math import dist2plane as ref_dist2plane  # noqa: E402

torch.set_num_threads(1)
ROWS, K, N = 9, 7, 5
SEED = 21
OWN_FP32_ERROR = 5e-7          # the reference's fp32 run against its own fp64 run, relative to max(1, max|fp64|)


def case_name(signed, scaled):
    return f"signed{int(signed)}_scaled{int(scaled)}"


def inputs():
    rng = np.random.default_rng(SEED)
    x = rng.standard_normal((ROWS, K))
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(0.05, 0.8, (ROWS, 1))
    # the planes as the layer initialises them (hyrnn_nets.py:219-225): p = expmap0(randn / 4), a = unit rows
    u = rng.standard_normal((N, K)) / 4
    un = np.linalg.norm(u, axis=1, keepdims=True)
    p = np.tanh(un) * u / un
    a = rng.standard_normal((N, K))
    a = a / np.linalg.norm(a, axis=1, keepdims=True)
    x[3] = 0.0
    x[5] *= 0.9 / np.linalg.norm(x[5])
    x[7] = p[2]
    scale = rng.standard_normal(N) * 0.3
    go = rng.standard_normal((ROWS, N)) / (ROWS * N)
    return {k: v.astype(np.float32) for k, v in dict(x=x, p=p, a=a, scale=scale, grad_output=go).items()}


def write_npz(path, arrays):
    """np.savez with the members' time stamps pinned (numpy stamps them with the wall clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def _own_error(got32, tensors64, kink=False):
    """Largest distance of the reference's fp32 arrays from its own fp64 arrays.  kink: without row 7 of grad_x and plane 2 of grad_p /
    grad_a -- row 7 lies ON plane 2, where the unsigned distance has its kink and the sign of that pair's gradient is rounding noise."""
    worst = 0.0
    for i, (g32, g64) in enumerate(zip(got32, tensors64)):
        g64 = g64.detach().numpy()
        if kink and i > 0:
            g32, g64 = np.delete(g32, 7 if i == 1 else 2, axis=0), np.delete(g64, 7 if i == 1 else 2, axis=0)
        worst = max(worst, float(np.abs(g32.astype(np.float64) - g64).max()) / max(1.0, float(np.abs(g64).max())))
    return worst


def _fp64_run(out, signed, scaled, with_scale):
    x, p, a, scale = (torch.from_numpy(out[n].astype(np.float64)).requires_grad_(True) for n in ("x", "p", "a", "scale"))
    o = ref_dist2plane(x.unsqueeze(-2), p, a, k=torch.tensor(-1.0, dtype=torch.float64), signed=signed, scaled=scaled)
    if with_scale:
        o = o * scale.exp()
    return [o] + list(torch.autograd.grad(o, [x, p, a] + ([scale] if with_scale else []), torch.from_numpy(out["grad_output"]).double()))


def main():
    out = inputs()
    T = lambda n: torch.from_numpy(out[n].copy()).requires_grad_(True)
    go = torch.from_numpy(out["grad_output"])
    k = torch.tensor(-1.0)
    for signed in (False, True):
        for scaled in (False, True):
            x, p, a = T("x"), T("p"), T("a")
            o = ref_dist2plane(x.unsqueeze(-2), p, a, k=k, signed=signed, scaled=scaled)
            assert o.shape == (ROWS, N)
            gs = torch.autograd.grad(o, [x, p, a], go)
            name = case_name(signed, scaled)
            out[f"{name}.out"] = o.detach().numpy()
            out[f"{name}.grad_x"], out[f"{name}.grad_p"], out[f"{name}.grad_a"] = (g.numpy() for g in gs)
            own = _own_error([out[f"{name}.{q}"] for q in ("out", "grad_x", "grad_p", "grad_a")], _fp64_run(out, signed, scaled, False),
                             kink=not signed)
            assert own <= OWN_FP32_ERROR, (name, own)
    x, p, a, scale = T("x"), T("p"), T("a"), T("scale")
    o = ref_dist2plane(x.unsqueeze(-2), p, a, k=k, signed=True) * scale.exp()          # hyrnn_nets.py:234-237
    gs = torch.autograd.grad(o, [x, p, a, scale], go)
    out["layer.out"] = o.detach().numpy()
    out["layer.grad_x"], out["layer.grad_p"], out["layer.grad_a"], out["layer.grad_scale"] = (g.numpy() for g in gs)
    own = _own_error([out[f"layer.{q}"] for q in ("out", "grad_x", "grad_p", "grad_a", "grad_scale")], _fp64_run(out, True, False, True))
    assert own <= OWN_FP32_ERROR, ("layer", own)
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "mobius_dist2plane.npz"), out)
    print("mobius_dist2plane.npz written:", len(out), "arrays")


if __name__ == "__main__":
    main()
