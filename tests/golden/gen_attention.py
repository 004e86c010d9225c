#!/usr/bin/env python3
"""Generate tests/golden/attention.npz by running the REFERENCE's own ``dist_matmul`` (math_.py:905-947), ``torch.softmax`` and
``weighted_midpoint_bmm`` (math_.py:2090-2122, imported through tests/golden/refharness.py) as one chain at k = -1:

    weighted_midpoint_bmm(values, softmax(-beta dist_matmul(q, keys^T) + bias, -1), k, lincomb=False)

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_attention.py

(batch, N, M, D, E) = (2, 5, 7, 3, 4), points within radius 0.8, beta = 1.7: q (2, 5, 3), keys (2, 7, 3), values (2, 7, 4); query
(1, 3) at norm 0.9, value row (0, 4) all zero; ``main`` asserts that no query and key of a batch element are closer than 0.05 in
Euclidean distance, so that no distance is the difference of nearly equal sums.  Two cases: ``plain`` without a bias, ``bias`` with
an N(0, 1) bias (2, 5, 7) that holds one -inf, at (1, 2, 5).

For each case the output and the autograd gradients of q, keys and values under one fixed grad_output -- that of a mean-reduced loss
with N(0, 1) weights, N(0, 1) / out.numel() -- are recorded: arrays only.  ``main`` asserts that the reference's fp32 run lies within
``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative to max(1, max|fp64|), and prints the worst values; no
restatement can be held closer to the records than that.  The archive is written with fixed member time stamps, so a second run
reproduces the file bit for bit.
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
SEED = 12
OWN_FP32_ERROR = 1e-6
BATCH, N, M, D, E = 2, 5, 7, 3, 4
BETA = 1.7
RIM_Q, ZERO_V, MASKED = (1, 3), (0, 4), (1, 2, 5)
MIN_SEPARATION = 0.05
LABELS = ("out", "grad_q", "grad_keys", "grad_values")


def _ball(rng, shape, radius):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True) * rng.uniform(0.05, radius, shape[:-1] + (1,))


def inputs():
    rng = np.random.default_rng(SEED)
    q, keys, values = _ball(rng, (BATCH, N, D), 0.8), _ball(rng, (BATCH, M, D), 0.8), _ball(rng, (BATCH, M, E), 0.8)
    q[RIM_Q] *= 0.9 / np.linalg.norm(q[RIM_Q])
    values[ZERO_V] = 0.0
    bias = rng.standard_normal((BATCH, N, M))
    bias[MASKED] = -np.inf
    out = dict(q=q, keys=keys, values=values, bias=bias, grad_output=rng.standard_normal((BATCH, N, E)) / (BATCH * N * E))
    return {k: v.astype(np.float32) for k, v in out.items()}


def write_npz(path, arrays):
    """np.savez with the members' time stamps pinned (numpy stamps them with the wall clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def _run(arrays, with_bias, dt):
    q, keys, values = (torch.from_numpy(arrays[n].astype(np.float64)).to(dt).requires_grad_(True) for n in ("q", "keys", "values"))
    k = torch.tensor(-1.0, dtype=dt)
    s = -BETA * ref.dist_matmul(q, keys.transpose(-1, -2), k)
    if with_bias:
        s = s + torch.from_numpy(arrays["bias"].astype(np.float64)).to(dt)
    o = ref.weighted_midpoint_bmm(values, torch.softmax(s, -1), k, lincomb=False)
    gs = torch.autograd.grad(o, [q, keys, values], torch.from_numpy(arrays["grad_output"].astype(np.float64)).to(dt))
    return [o.detach()] + list(gs)


def main():
    out = inputs()
    worst = {}
    sep = np.linalg.norm(out["q"].astype(np.float64)[:, :, None, :] - out["keys"].astype(np.float64)[:, None, :, :], axis=-1)
    assert float(sep.min()) >= MIN_SEPARATION, float(sep.min())
    for name, with_bias in (("plain", False), ("bias", True)):
        r32, r64 = _run(out, with_bias, torch.float32), _run(out, with_bias, torch.float64)
        for lab, a32, a64 in zip(LABELS, r32, r64):
            assert bool(torch.isfinite(a32).all()) and bool(torch.isfinite(a64).all()), (name, lab)
            own = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
            assert own <= OWN_FP32_ERROR, (name, lab, own)
            worst[f"{name}.{lab}"] = own
            out[f"{name}.{lab}"] = a32.numpy()
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "attention.npz"), out)
    w = max(worst, key=worst.get)
    print("attention.npz written:", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")


if __name__ == "__main__":
    main()
