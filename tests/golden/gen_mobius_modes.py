#!/usr/bin/env python3
"""Generate tests/golden/mobius_modes.npz by running the REFERENCE's own ``hyperspace.hyrnn_nets.mobius_linear`` and
``mobius_matvec`` (imported through tests/golden/refharness.py) in fp32 on one small input.

Run in the build container only (it needs the reference tree):

    PYTORCH_JIT=0 PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_mobius_modes.py

Cases: hyperbolic_input x hyperbolic_bias x (bias | no bias) -- eight -- times nonlin in (None, torch.tanh, torch.relu), plus the
bare mobius_matvec.  9 rows, K = 7, N = 5; row 3 is all zero, row 5 has norm 0.9.  For every case the output and the gradients of
x, weight and bias under one fixed grad_output are recorded -- arrays only.  The archive is written with fixed member time stamps,
so a second run reproduces the file bit for bit.
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

from hyperspace.hyrnn_nets import mobius_linear as ref_mobius_linear  # noqa: E402
from hyperspace.hyrnn_nets import mobius_matvec as ref_mobius_matvec  # noqa: E402

torch.set_num_threads(1)
ROWS, K, N = 9, 7, 5
NONLINS = {"none": None, "tanh": torch.tanh, "relu": torch.relu}


def case_name(hyperbolic_input, hyperbolic_bias, with_bias, nonlin):
    return f"hi{int(hyperbolic_input)}_hb{int(hyperbolic_bias)}_b{int(with_bias)}_{nonlin}"


def inputs():
    rng = np.random.default_rng(20)
    x = rng.standard_normal((ROWS, K))
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * rng.uniform(0.05, 0.8, (ROWS, 1))
    x[3] = 0.0
    x[5] *= 0.9 / np.linalg.norm(x[5])
    w = rng.standard_normal((N, K)) * 0.4
    b = rng.standard_normal(N)
    bias_ball = b / np.linalg.norm(b) * 0.3
    bias_eucl = rng.standard_normal(N) * 0.3
    go = rng.standard_normal((ROWS, N))
    return {k: v.astype(np.float32) for k, v in dict(x=x, weight=w, bias_ball=bias_ball, bias_eucl=bias_eucl, grad_output=go).items()}


def write_npz(path, arrays):
    """np.savez with the members' time stamps pinned (numpy stamps them with the wall clock)."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def main():
    out = inputs()
    T = lambda a: torch.from_numpy(out[a].copy()).requires_grad_(True)
    go = torch.from_numpy(out["grad_output"])
    for hi in (False, True):
        for hb in (False, True):
            for with_bias in (False, True):
                for tag, fn in NONLINS.items():
                    x, w = T("x"), T("weight")
                    b = T("bias_ball" if hb else "bias_eucl") if with_bias else None
                    o = ref_mobius_linear(x, w, b, hyperbolic_input=hi, hyperbolic_bias=hb, nonlin=fn, k=-1.0)
                    gs = torch.autograd.grad(o, [x, w] + ([b] if with_bias else []), go)
                    name = case_name(hi, hb, with_bias, tag)
                    out[f"{name}.out"] = o.detach().numpy()
                    out[f"{name}.grad_x"], out[f"{name}.grad_weight"] = gs[0].numpy(), gs[1].numpy()
                    if with_bias:
                        out[f"{name}.grad_bias"] = gs[2].numpy()
    x, w = T("x"), T("weight")
    o = ref_mobius_matvec(w, x, k=torch.tensor(-1.0))
    gs = torch.autograd.grad(o, [x, w], go)
    out["matvec.out"], out["matvec.grad_x"], out["matvec.grad_weight"] = o.detach().numpy(), gs[0].numpy(), gs[1].numpy()
    assert all(v.dtype == np.float32 for v in out.values())
    write_npz(os.path.join(HERE, "mobius_modes.npz"), out)
    print("mobius_modes.npz written:", len(out), "arrays")


if __name__ == "__main__":
    main()
