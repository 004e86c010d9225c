#!/usr/bin/env python3
"""Generate tests/golden/weighted_midpoint.npz by running the REFERENCE's own ``weighted_midpoint``, ``weighted_midpoint_bmm`` and
``mobius_scalar_mul`` (math_.py:1953-2122, :788-858, imported through tests/golden/refharness.py) in fp32 at k = -1.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_weighted_midpoint.py

bmm form, (batch, N, M, D) = (2, 5, 7, 3): xs within radius 0.8, row (0, 2) all zero, row (1, 4) at norm 0.9; weights ``softmax`` (a
softmax over M), ``signed`` (N(0, 1) / 2) and ``zerow`` (the signed ones with row (1, 3) all zero: den = 0 sits on its clamp 1e-10, the
output row is 0 and grad_w of that row is grad_t * 1e10 -- in a case of its own, so that the other cases' gradients are not measured
against that size); each with lincomb off and on.
reduce form, xs (6, 9, 5) within radius 0.6, row (2, 4) all zero, row (3, 1) at norm 0.9: the cases of ``REDUCE_CASES``.
mobius_scalar_mul, x (9, 5) within radius 0.8, row 3 all zero: r per row (9, 1) in [-1.5, 2.5] and one r = 1.7.  grad_x of the zero
row is recorded but held to nothing: there the gradient is g tanh(r artanh(1e-15)) / 1e-15, and artanh(1e-15) -- the difference of
log(1 + 1e-15) and log(1 - 1e-15) -- is 0 in fp32 and 1e-15 in fp64, so the reference returns 0 in fp32 and r g in fp64.

For every case the output and the autograd gradients of every operand under one fixed grad_output -- that of a mean-reduced loss with
N(0, 1) weights, N(0, 1) / out.numel() -- are recorded: arrays only.  ``main`` asserts that the reference's fp32 run lies within
``OWN_FP32_ERROR`` = 1e-6 of its own fp64 run on every recorded array, relative to max(1, max|fp64|), and prints the worst value; no
restatement can be held closer to the records than that.  (Its fp64 run projects at 1 - 1e-5, its fp32 run at 1 - 4e-3: ``main``
asserts that no bmm output comes near either, so the two runs compute the same function.)  The archive is written with fixed member
time stamps, so a second run reproduces the file bit for bit.
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
RM, RR, RD = 6, 9, 5
SMUL_ZERO_ROW = 3
BMM_KINDS = ("softmax", "signed", "zerow")
# name: (reducedim, keepdim, weights, posweight, lincomb, coadd)
REDUCE_CASES = {
    "r0_none": ([0], False, None, False, False, False),
    "r0_pos": ([0], False, "pos", False, False, False),
    "r0_signed": ([0], False, "signed", False, False, False),
    "all_pos": (None, False, "pos", False, False, False),
    "all_none_lincomb": (None, False, None, False, True, False),
    "r0_pos_keepdim": ([0], True, "pos", False, False, False),
    "r0_signed_posweight": ([0], False, "signed", True, False, False),
    "r0_signed_lincomb": ([0], False, "signed", False, True, False),
    "r0_signed_posweight_lincomb": ([0], False, "signed", True, True, False),
    "r0_signed_coadd": ([0], False, "signed", False, False, True),
    "r0_scalar_lincomb": ([0], False, "scalar", False, True, False),
}


def _ball(rng, shape, radius):
    x = rng.standard_normal(shape)
    return x / np.linalg.norm(x, axis=-1, keepdims=True) * rng.uniform(0.05, radius, shape[:-1] + (1,))


def inputs():
    rng = np.random.default_rng(SEED)
    xs = _ball(rng, (BATCH, M, D), 0.8)
    xs[0, 2] = 0.0
    xs[1, 4] *= 0.9 / np.linalg.norm(xs[1, 4])
    logits = rng.standard_normal((BATCH, N, M))
    e = np.exp(logits - logits.max(-1, keepdims=True))
    signed = rng.standard_normal((BATCH, N, M)) / 2
    zerow = signed.copy()
    zerow[1, 3] = 0.0
    rx = _ball(rng, (RM, RR, RD), 0.6)
    rx[2, 4] = 0.0
    rx[3, 1] *= 0.9 / np.linalg.norm(rx[3, 1])
    sx = _ball(rng, (9, 5), 0.8)
    sx[SMUL_ZERO_ROW] = 0.0
    out = dict(bmm_xs=xs, bmm_w_softmax=e / e.sum(-1, keepdims=True), bmm_w_signed=signed, bmm_w_zerow=zerow,
               bmm_grad_output=rng.standard_normal((BATCH, N, D)) / (BATCH * N * D),
               red_xs=rx, red_w_pos=rng.uniform(0.1, 1.0, (RM, RR)), red_w_signed=rng.uniform(-1.0, 1.0, (RM, RR)), red_w_scalar=np.array(0.7),
               red_grad_output_r0=rng.standard_normal((RR, RD)) / (RR * RD), red_grad_output_all=rng.standard_normal((RD,)) / RD,
               smul_x=sx, smul_r_rows=rng.uniform(-1.5, 2.5, (9, 1)), smul_r_scalar=np.array(1.7), smul_grad_output=rng.standard_normal((9, 5)) / 45)
    return {k: v.astype(np.float32) for k, v in out.items()}


def bmm_name(kind, lincomb):
    return f"bmm_{kind}_lincomb{int(lincomb)}"


def write_npz(path, arrays):
    """np.savez with the members' time stamps pinned (numpy stamps them with the wall clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def _run(fn, operands, go, dt):
    """fn on leaves of dtype dt: [out, grad of every operand that is not None]."""
    leaves = [None if a is None else torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True) for a in operands]
    o = fn(*leaves, torch.tensor(-1.0, dtype=dt))
    gs = torch.autograd.grad(o, [t for t in leaves if t is not None], torch.from_numpy(go.astype(np.float64)).to(dt).reshape(o.shape))
    return [o.detach()] + list(gs)


def _record(out, worst, name, labels, fn, operands, go, skip=None):
    """skip = (label, row): that row of that array is recorded but not held to the fp64 run."""
    r32, r64 = _run(fn, operands, go, torch.float32), _run(fn, operands, go, torch.float64)
    for lab, a32, a64 in zip(labels, r32, r64):
        d = (a32.double() - a64).abs()
        if skip and skip[0] == lab:
            d[skip[1]] = 0
        own = float(d.max()) / max(1.0, float(a64.abs().max()))
        assert own <= OWN_FP32_ERROR, (name, lab, own)
        worst[f"{name}.{lab}"] = own
        out[f"{name}.{lab}"] = a32.numpy()
    return r64[0]


def main():
    out = inputs()
    worst = {}
    for kind in BMM_KINDS:
        for lincomb in (False, True):
            o64 = _record(out, worst, bmm_name(kind, lincomb), ("out", "grad_xs", "grad_w"),
                          lambda x, w, k, lc=lincomb: ref.weighted_midpoint_bmm(x, w, k, lincomb=lc),
                          (out["bmm_xs"], out[f"bmm_w_{kind}"]), out["bmm_grad_output"])
            assert float(o64.norm(dim=-1).max()) < 0.99, "a bmm output reaches project's sphere: the fp32 and fp64 runs would differ by construction"
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in REDUCE_CASES.items():
        go = out["red_grad_output_all" if reducedim is None else "red_grad_output_r0"]
        fn = lambda x, w, k: ref.weighted_midpoint(x, k, weights=w, reducedim=reducedim, keepdim=keepdim, lincomb=lincomb, posweight=posweight,
                                                   coadd=coadd)
        o64 = _record(out, worst, "red_" + name, ("out", "grad_xs") + (() if wk is None else ("grad_w",)), fn,
                      (out["red_xs"], None if wk is None else out[f"red_w_{wk}"]), go)
        assert tuple(o64.shape) == ((RD,) if reducedim is None else (1, RR, RD) if keepdim else (RR, RD)), (name, o64.shape)
    for name, r in (("smul_rows", out["smul_r_rows"]), ("smul_scalar", out["smul_r_scalar"])):
        _record(out, worst, name, ("out", "grad_r", "grad_x"), lambda rr, x, k: ref.mobius_scalar_mul(rr, x, k=k), (r, out["smul_x"]),
                out["smul_grad_output"], skip=("grad_x", SMUL_ZERO_ROW))
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "weighted_midpoint.npz"), out)
    w = max(worst, key=worst.get)
    print("weighted_midpoint.npz written:", len(out), "arrays; the reference's fp32 run against its fp64 run, worst", f"{worst[w]:.2e}", "at", w)
    for grp in ("bmm", "red", "smul"):
        print(" ", grp, f"{max(v for k, v in worst.items() if k.startswith(grp)):.2e}")


if __name__ == "__main__":
    main()
