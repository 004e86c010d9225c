"""Hyperbolic attention on the host: the restatement of tests/attention_ref.py against the reference's own recorded outputs
(tests/golden/attention.npz, written by tests/golden/gen_attention.py), the backward formulas the kernels run against autograd of the
restatement, the C ABI's declarations and bindings, and the refusals of the Python function -- which come before any device call, so
they run here.

The bounds.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative
to max(1, max|array|) (measured worst: 1.04e-7, plain.out); the restatement is held to the fp32 records at the same 1e-6, run in fp64
and in fp32.  The backward formulas are algebra on the same fp64 numbers as autograd's chain, sums of at most 7 terms of size <= 10:
held to 1e-12 relative to max(1, max|gradient|) (measured: 2e-16).
"""
import os
import re

import numpy as np
import pytest
import torch

from attention_ref import attention_backward_formulas, hyperbolic_attention_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6
FORMULA_BOUND = 1e-12
BETA = 1.7
RIM_Q, ZERO_V, MASKED = (1, 3), (0, 4), (1, 2, 5)       # the generator's named cases
LABELS = ("out", "grad_q", "grad_keys", "grad_values")
NEW_ENTRY_POINTS = ("hypad_hyp_attention_fwd", "hypad_hyp_attention_workspace_bytes", "hypad_hyp_attention_bwd")


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "attention.npz")) as z:
        return {k: z[k] for k in z.files}


def _leaves(fx, dt):
    return [torch.from_numpy(fx[k].astype(np.float64)).to(dt).requires_grad_(True) for k in ("q", "keys", "values")]


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_recorded_reference(dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 for v in fx.values())
    for name in ("plain", "bias"):
        leaves = _leaves(fx, dt)
        bias = torch.from_numpy(fx["bias"].astype(np.float64)).to(dt) if name == "bias" else None
        o = hyperbolic_attention_ref(*leaves, BETA, bias)
        assert tuple(o.shape) == fx[f"{name}.out"].shape
        gs = torch.autograd.grad(o, leaves, torch.from_numpy(fx["grad_output"].astype(np.float64)).to(dt))
        for lab, got in zip(LABELS, [o.detach()] + list(gs)):
            rec = fx[f"{name}.{lab}"].astype(np.float64)
            err = float(np.abs(got.double().numpy() - rec).max()) / max(1.0, float(np.abs(rec).max()))
            assert err <= BOUND, (name, lab, str(dt), err)


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    q, keys, values, bias = fx["q"], fx["keys"], fx["values"], fx["bias"]
    assert q.shape == (2, 5, 3) and keys.shape == (2, 7, 3) and values.shape == (2, 7, 4) and bias.shape == (2, 5, 7)
    assert all(fx[f"{c}.out"].shape == (2, 5, 4) and fx[f"{c}.grad_values"].shape == (2, 7, 4) for c in ("plain", "bias"))
    assert abs(float(np.linalg.norm(q[RIM_Q])) - 0.9) < 1e-6 and not values[ZERO_V].any()
    assert np.isneginf(bias[MASKED]) and int(np.isinf(bias).sum()) == 1
    sep = np.linalg.norm(q[:, :, None, :].astype(np.float64) - keys[:, None, :, :], axis=-1)
    assert float(sep.min()) >= 0.05
    for a in (q, keys, values):
        assert float(np.linalg.norm(a, axis=-1).max()) <= 0.9 + 1e-6
    assert all(np.isfinite(v).all() for k, v in fx.items() if k != "bias")
    assert not np.array_equal(fx["plain.out"], fx["bias.out"])


def _rel(got, want):
    return float((got - want).abs().max()) / max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("case", ["plain", "one -inf", "a masked row"])
def test_backward_formulas_meet_autograd_of_the_restatement(case):
    fx = load_fixture()
    q, keys, values = _leaves(fx, torch.float64)
    bias = None if case == "plain" else torch.from_numpy(fx["bias"].astype(np.float64))
    if case == "a masked row":
        bias[0, 4, :] = -np.inf
    go = torch.randn(2, 5, 4, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    out = hyperbolic_attention_ref(q, keys, values, BETA, bias)
    assert bool(torch.isfinite(out).all())
    want = torch.autograd.grad(out, [q, keys, values], go)
    got = attention_backward_formulas(q.detach(), keys.detach(), values.detach(), go, BETA, bias)
    for lab, g, w in zip(LABELS[1:], got, want):
        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(g).all()), (case, lab)
        err = _rel(g, w)
        print(f"\nbackward formulas, {case}, {lab}: {err:.1e}")
        assert err <= FORMULA_BOUND, (case, lab, err)
    if case == "a masked row":
        assert not out[0, 4].any() and not want[0][0, 4].any() and not got[0][0, 4].any()


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert re.search(r"#define HYPAD_ABI_VERSION 7\b", text)
    assert re.search(r"\bsize_t hypad_hyp_attention_workspace_bytes\(", text)
    for name in ("hypad_hyp_attention_fwd", "hypad_hyp_attention_bwd"):
        assert re.search(r"\bint " + name + r"\(", text), name
    entry = text[text.index("gmath.hyperbolic_attention"):text.index("size_t hypad_hyp_attention_workspace_bytes(")]
    assert "math_.py:905-947" in entry and "math_.py:2090-2122" in entry and "bias_batch_stride" in entry
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes is not None, name
    assert len(_C._SIGS["hypad_hyp_attention_workspace_bytes"][1]) == 5
    assert len(_C._SIGS["hypad_hyp_attention_fwd"][1]) == 15 and len(_C._SIGS["hypad_hyp_attention_bwd"][1]) == 20


def test_export_map_and_source_list_carry_the_new_file():
    from hypad_amd import build
    assert "attention.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "attention.hip"))
    assert "global: hypad_*;" in open(os.path.join(build.CSRC, "exports.map")).read()
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", build.LIB], capture_output=True, text=True, check=True).stdout
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bT " + name + r"\b", syms), name


def test_entry_points_validate_sizes_before_any_hip_call():
    """Host pointers and no device: every answer below comes from the checks that run before the first HIP call."""
    import ctypes
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    EINVAL, EUNSUPPORTED = -1, -3

    def fwd(b=2, n=4, m=6, d=8, e=8, beta=1.0, q=p, stride=0):
        return L.hypad_hyp_attention_fwd(q, p, p, None, stride, beta, p, None, None, b, n, m, d, e, None)

    def bwd(b=2, n=4, m=6, d=8, e=8, beta=1.0):
        return L.hypad_hyp_attention_bwd(p, p, p, None, 0, beta, p, p, p, p, p, p, p, 1 << 20, b, n, m, d, e, None)

    for call in (fwd, bwd):
        assert call(b=-1) == call(n=-1) == call(m=-2) == call(d=0) == call(e=0) == call(d=-3) == call(m=0) == EINVAL
        assert call(beta=float("inf")) == call(beta=float("nan")) == EINVAL
        assert call(d=129) == call(e=129) == call(b=1, n=2 ** 16, m=2 ** 15) == call(b=2 ** 20, n=2 ** 6, m=2 ** 5) == EUNSUPPORTED
    assert fwd(b=0) == 0 and fwd(n=0) == 0 and fwd(n=0, m=0) == 0
    assert L.hypad_hyp_attention_workspace_bytes(2, 4, 6, 8, 10) == 4 * 2 * 4 * 12 and L.hypad_hyp_attention_workspace_bytes(2, 0, 6, 8, 10) == 0


def test_python_function_refuses_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    att = gmath.hyperbolic_attention
    q, keys, values, bias = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.zeros(2, 7, 4), torch.zeros(2, 5, 7)
    refused = [lambda k=k: att(q, keys, values, k) for k in (-0.5, 1.0, 0.0)]
    refused += [lambda: att(q.double(), keys, values, -1.0), lambda: att(q, keys.double(), values, -1.0), lambda: att(q, keys, values.double(), -1.0),
                lambda: att(q, keys, values, -1.0, bias=bias.double()), lambda: att(q.half(), keys.half(), values.half(), -1.0)]
    # D or E above 128 (with the unfused composition named), below 1; no keys
    refused += [lambda: att(torch.zeros(2, 5, 129), torch.zeros(2, 7, 129), values, -1.0), lambda: att(q, keys, torch.zeros(2, 7, 129), -1.0),
                lambda: att(torch.zeros(2, 5, 0), torch.zeros(2, 7, 0), values, -1.0), lambda: att(q, keys, torch.zeros(2, 7, 0), -1.0),
                lambda: att(q, torch.zeros(2, 0, 3), torch.zeros(2, 0, 4), -1.0)]
    # operands that do not fit each other
    refused += [lambda: att(q, torch.zeros(2, 7, 4), values, -1.0), lambda: att(q, keys, torch.zeros(2, 6, 4), -1.0),
                lambda: att(q, torch.zeros(3, 7, 3), values, -1.0), lambda: att(torch.zeros(4, 2, 5, 3), keys, values, -1.0),
                lambda: att(torch.zeros(3), keys, values, -1.0), lambda: att(q, keys, torch.zeros(4), -1.0),
                lambda: att(q, keys, values, -1.0, bias=torch.zeros(5, 6)), lambda: att(q, keys, values, -1.0, bias=torch.zeros(3, 5, 7)),
                lambda: att(q, keys, values, -1.0, bias=torch.zeros(7)), lambda: att(q[0], keys[0], values[0], -1.0, bias=bias)]
    # bias or beta requiring grad, a beta that is not finite or not one element
    refused += [lambda: att(q, keys, values, -1.0, bias=bias.clone().requires_grad_(True)),
                lambda: att(q, keys, values, -1.0, beta=torch.ones(1, requires_grad=True)), lambda: att(q, keys, values, -1.0, beta=torch.ones(2)),
                lambda: att(q, keys, values, -1.0, beta=float("inf")), lambda: att(q, keys, values, -1.0, beta=float("nan")),
                lambda: att(q, keys, values, -1.0, beta=torch.tensor(float("-inf")))]
    # 2^31 pairs
    refused += [lambda: att(torch.zeros(1, 1).expand(65536, 1), torch.zeros(1, 1).expand(32768, 1), torch.zeros(1, 1).expand(32768, 1), -1.0)]
    for i, call in enumerate(refused):
        with pytest.raises(NotImplementedError, match="supported"):
            call()
    with pytest.raises(NotImplementedError, match="dist_matmul, torch.softmax and weighted_midpoint_bmm"):
        att(torch.zeros(2, 5, 129), torch.zeros(2, 7, 129), values, -1.0)
    # what is supported gets as far as the device and is refused there, on a host without one
    for call in (lambda: att(q, keys, values, -1.0), lambda: att(q[0], keys, values, -1.0, beta=torch.tensor(2.0)), lambda: att(q, keys[0], values[0], None),
                 lambda: att(q, keys, values, -1.0, beta=0.5, bias=bias), lambda: att(q, keys, values, -1.0, bias=bias[0]),
                 lambda: att(q.reshape(2, 1, 5, 3), keys.reshape(2, 1, 7, 3), values[0], torch.tensor(-1.0), bias=bias.reshape(2, 1, 5, 7))):
        with pytest.raises(_C.HypadError, match="GPU"):
            call()
