#!/usr/bin/env python3
"""Generate tests/golden/dist.npz by running the REFERENCE's own ``dist_matmul``, ``dist`` and ``dist0`` (math_.py:905-947, :861-902,
:950-975, imported through tests/golden/refharness.py) in fp32 at k = -1.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_dist.py

Pair form, (batch, N, M, D) = (2, 5, 7, 3), points within radius 0.8: x (2, 5, 3) and y in the reference's layout (2, 3, 7); x row
(1, 3) at norm 0.9; x row (0, 2) and y point (0, 4) all zero -- that pair is 2 artanh(sqrt(1e-15)) = 6.3e-8 whatever the rounding of
the sums (the reference's fp32 artanh, a difference of two logarithms, returns 0 for it) and gets no gradient: ``u`` sits on its
clamp --; ``main`` asserts that no other pair of a batch element is closer than 0.05 in Euclidean distance,
so that no recorded distance is the difference of nearly equal sums.
Row forms, x and y (9, 5) within radius 0.8: x row 1 and y row 2 all zero, row 3 zero in both, row 4 the same point in both (norm 0.6:
above norm 0.5 the coefficients 1 - 2 |x|^2 + |x|^2 and 1 - |x|^2 of (-x) (+) x agree to the bit in fp32 and fp64 alike, so the
reference returns distance 0 and gradient 0, which ``main`` asserts), x row 5 at norm 0.9.  dist0 runs on the same x.

For every case the output and the autograd gradients of every operand under one fixed grad_output -- that of a mean-reduced loss with
N(0, 1) weights, N(0, 1) / out.numel() -- are recorded: arrays only.  ``main`` asserts that the reference's fp32 run lies within
``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative to max(1, max|fp64|), and prints the worst value; no
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
SEED = 7
OWN_FP32_ERROR = 1e-6
BATCH, N, M, D = 2, 5, 7, 3
ROWS, RD = 9, 5
PAIR_RIM_X, PAIR_ZERO_X, PAIR_ZERO_Y = (1, 3), (0, 2), (0, 4)
ROW_ZERO_X, ROW_ZERO_Y, ROW_ZERO_BOTH, ROW_EQUAL, ROW_RIM = 1, 2, 3, 4, 5
MIN_SEPARATION = 0.05


def _ball(rng, shape, radius):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True) * rng.uniform(0.05, radius, shape[:-1] + (1,))


def inputs():
    rng = np.random.default_rng(SEED)
    x = _ball(rng, (BATCH, N, D), 0.8)
    yp = _ball(rng, (BATCH, M, D), 0.8)                     # points (batch, M, D)
    x[PAIR_RIM_X] *= 0.9 / np.linalg.norm(x[PAIR_RIM_X])
    x[PAIR_ZERO_X] = 0.0
    yp[PAIR_ZERO_Y] = 0.0
    rx, ry = _ball(rng, (ROWS, RD), 0.8), _ball(rng, (ROWS, RD), 0.8)
    rx[ROW_ZERO_X] = 0.0
    ry[ROW_ZERO_Y] = 0.0
    rx[ROW_ZERO_BOTH] = ry[ROW_ZERO_BOTH] = 0.0
    rx[ROW_EQUAL] *= 0.6 / np.linalg.norm(rx[ROW_EQUAL])
    rx[ROW_RIM] *= 0.9 / np.linalg.norm(rx[ROW_RIM])
    out = dict(dm_x=x, dm_y=np.ascontiguousarray(np.swapaxes(yp, -1, -2)), dm_grad_output=rng.standard_normal((BATCH, N, M)) / (BATCH * N * M),
               row_x=rx, row_y=ry, row_grad_output=rng.standard_normal((ROWS,)) / ROWS)
    out = {k: v.astype(np.float32) for k, v in out.items()}
    out["row_y"][ROW_EQUAL] = out["row_x"][ROW_EQUAL]       # (equal as stored)
    return out


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


def _record(out, worst, name, labels, fn, operands, go):
    r32, r64 = _run(fn, operands, go, torch.float32), _run(fn, operands, go, torch.float64)
    for lab, a32, a64 in zip(labels, r32, r64):
        own = float((a32.double() - a64).abs().max()) / max(1.0, float(a64.abs().max()))
        assert own <= OWN_FP32_ERROR, (name, lab, own)
        worst[f"{name}.{lab}"] = own
        out[f"{name}.{lab}"] = a32.numpy()
    return r32, r64


def main():
    out = inputs()
    worst = {}
    x, yp = out["dm_x"].astype(np.float64), np.swapaxes(out["dm_y"], -1, -2).astype(np.float64)
    sep = np.linalg.norm(x[:, :, None, :] - yp[:, None, :, :], axis=-1)
    sep[PAIR_ZERO_X[0], PAIR_ZERO_X[1], PAIR_ZERO_Y[1]] = np.inf
    assert float(sep.min()) >= MIN_SEPARATION, float(sep.min())
    r32, r64 = _record(out, worst, "dm", ("out", "grad_x", "grad_y"), lambda a, b, k: ref.dist_matmul(a, b, k), (out["dm_x"], out["dm_y"]),
                       out["dm_grad_output"])
    zz = 2 * np.arctanh(np.sqrt(1e-15))
    at = (PAIR_ZERO_X[0], PAIR_ZERO_X[1], PAIR_ZERO_Y[1])
    assert abs(float(r64[0][at]) - zz) <= 1e-6 * zz and 0.0 <= float(r32[0][at]) <= 1.01 * zz
    runs = _record(out, worst, "dist", ("out", "grad_x", "grad_y"), lambda a, b, k: ref.dist(a, b, k=k), (out["row_x"], out["row_y"]),
                   out["row_grad_output"])
    for r in runs:                                          # the equal pair and the pair of zero rows: distance 0, gradient 0
        for row in (ROW_EQUAL, ROW_ZERO_BOTH):
            assert float(r[0][row]) == 0.0 and not r[1][row].any() and not r[2][row].any(), row
    runs = _record(out, worst, "dist0", ("out", "grad_x"), lambda a, k: ref.dist0(a, k=k), (out["row_x"],), out["row_grad_output"])
    for r in runs:
        assert float(r[0][ROW_ZERO_X]) == 0.0 and not r[1][ROW_ZERO_X].any()
    o = ref.dist(torch.from_numpy(out["row_x"]), torch.from_numpy(out["row_y"]), k=torch.tensor(-1.0), keepdim=True)
    assert tuple(o.shape) == (ROWS, 1)
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "dist.npz"), out)
    w = max(worst, key=worst.get)
    print("dist.npz written:", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for k in sorted(worst):
        print(" ", k, f"{worst[k]:.2e}")


if __name__ == "__main__":
    main()
