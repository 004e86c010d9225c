"""mobius_linear in every configuration and the Moebius matvec, restated in plain torch from ``oracle.gmath`` primitives, against
tests/golden/mobius_modes.npz -- the outputs and gradients of the reference's own ``hyperspace.hyrnn_nets.mobius_linear`` /
``mobius_matvec`` in fp32 (tests/golden/gen_mobius_modes.py).  The restatement is the yardstick of tests/test_gpu_mobius_modes.py,
which runs it in fp64 and fp32 on the CPU; here it is pinned to the reference itself: in fp64 and in fp32 it meets every recorded array
at 1e-6 (error relative to max(1, max|recorded|), as sweep_common.rel_err) -- but for one row of one gradient in two of the 24
configurations, where fp32 and fp64 part ways by construction (``_degenerate``) and only the fp32 run can be held to the record.
Also: the C ABI declares the five new entry points.
"""
import os
import re

import numpy as np
import pytest
import torch

import sweep_common as sc
from oracle import gmath as og

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mobius_modes.npz")
NONLINS = {"none": None, "tanh": torch.tanh, "relu": torch.relu}
NEW_ENTRY_POINTS = ("hypad_mobius_matvec_fwd", "hypad_mobius_matvec_bwd", "hypad_mobius_linear_ex_workspace_bytes",
                    "hypad_mobius_linear_ex_fwd", "hypad_mobius_linear_ex_bwd")


# ------------------------------------------------------------------------------------------------ the restatement
def mobius_matvec_ref(m, x):
    """hyperspace/hyrnn_nets.py:42-58 at k = -1 for a 2-D m: returns (M (x) x, mx = x M^T)."""
    x_norm = x.norm(dim=-1, keepdim=True, p=2).clamp_min(og.MIN_NORM)
    mx = x @ m.t()
    mx_norm = mx.norm(dim=-1, keepdim=True, p=2).clamp_min(og.MIN_NORM)
    res_c = og.tanh_clamped(mx_norm / x_norm * og.artanh(x_norm)) * (mx / mx_norm)
    cond = (mx == 0).all(dim=-1, keepdim=True)
    return torch.where(cond, torch.zeros((), dtype=res_c.dtype), res_c), mx


def mobius_fn_apply_ref(fn, x):
    """math_.py:1431-1469"""
    return og.expmap0(fn(og.logmap0(x)))


def mobius_linear_ref(x, w, bias_rows, hyperbolic_input, hyperbolic_bias, nonlin):
    """hyperspace/hyrnn_nets.py:13-35 at k = -1.  ``bias_rows``: None, or the bias expanded to one row per input row (so that the
    per-row bias gradients exist).  project takes the fp32 eps 4e-3 in fp64 too: the kernels' sphere.  Returns (out, mx)."""
    if hyperbolic_input:
        out, mx = mobius_matvec_ref(w, x)
    else:
        mx = torch.nn.functional.linear(x, w)
        out = og.expmap0(mx)
    if bias_rows is not None:
        out = og.mobius_add(out, bias_rows if hyperbolic_bias else og.expmap0(bias_rows))
    if nonlin is not None:
        out = mobius_fn_apply_ref(nonlin, out)
    return og.project(out, eps=og.PROJ_EPS_F32), mx


def case_name(hyperbolic_input, hyperbolic_bias, with_bias, nonlin):
    return f"hi{int(hyperbolic_input)}_hb{int(hyperbolic_bias)}_b{int(with_bias)}_{nonlin}"


CASES = [(hi, hb, wb, nl) for hi in (False, True) for hb in (False, True) for wb in (False, True) for nl in NONLINS]


def load_fixture():
    return dict(np.load(FIXTURE, allow_pickle=False))


# ------------------------------------------------------------------------------------------------ tests
def _meets(name, got, recorded, failures):
    err, i = sc.rel_err(got, recorded)
    if not err <= 1e-6:
        failures.append(f"{name}: {err:.3e} at flat index {i}")


def test_fixture_holds_every_configuration():
    fx = load_fixture()
    assert fx["x"].shape == (9, 7) and fx["weight"].shape == (5, 7)
    norms = np.linalg.norm(fx["x"].astype(np.float64), axis=1)
    assert (fx["x"] == 0).all(axis=1).sum() == 1 and abs(norms.max() - 0.9) < 1e-6
    for hi, hb, wb, nl in CASES:
        name = case_name(hi, hb, wb, nl)
        for part in ("out", "grad_x", "grad_weight") + (("grad_bias",) if wb else ()):
            assert fx[f"{name}.{part}"].dtype == np.float32, (name, part)
    assert all(v.dtype == np.float32 for v in fx.values())


def _degenerate(hi, wb, nl):
    """Euclidean input, no bias, tanh: the all-zero row of x reaches logmap0 as the zero row, where the reference's own fp32
    arithmetic and any fp64 restatement part ways by construction -- artanh(1e-15) = (log(1 + 1e-15) - log(1 - 1e-15)) / 2 is exactly 0
    in fp32 and 1.05e-15 in fp64, so logmap0 passes the fraction 0 of that row's gradient in fp32 and 1.05 of it in fp64 (the limit
    is 1).  The recorded grad_x row is exactly zero; the fp64 one is not (0.47 off on this input).  That one row of that one tensor
    is held to the fp32 restatement instead, which must give the reference's zeros; everything else is held to both."""
    return (not hi) and (not wb) and nl == "tanh"


@pytest.mark.parametrize("hi,hb,wb,nl", CASES, ids=lambda v: str(v))
def test_restatement_meets_the_reference(hi, hb, wb, nl):
    fx = load_fixture()
    name, failures = case_name(hi, hb, wb, nl), []
    for dt in (torch.float64, torch.float32):
        x, w = (torch.from_numpy(fx[k]).to(dt).requires_grad_(True) for k in ("x", "weight"))
        b = torch.from_numpy(fx["bias_ball" if hb else "bias_eucl"]).to(dt).requires_grad_(True) if wb else None
        out, _ = mobius_linear_ref(x, w, b.unsqueeze(0).expand(x.shape[0], -1) if wb else None, hi, hb, NONLINS[nl])
        grads = torch.autograd.grad(out, [x, w] + ([b] if wb else []), torch.from_numpy(fx["grad_output"]).to(dt))
        tag = "fp64" if dt == torch.float64 else "fp32"
        _meets(f"{tag} out", out, fx[f"{name}.out"], failures)
        for part, g in zip(("grad_x", "grad_weight", "grad_bias"), grads):
            rec = fx[f"{name}.{part}"]
            if part == "grad_x" and dt == torch.float64 and _degenerate(hi, wb, nl):
                assert (rec[3] == 0).all() and bool(torch.isfinite(g[3]).all())
                g, rec = np.delete(g.numpy(), 3, axis=0), np.delete(rec, 3, axis=0)
            _meets(f"{tag} {part}", g, rec, failures)
        if hi:                                      # the all-zero row: `cond`
            assert bool((grads[0][3] == 0).all()) and (fx[f"{name}.grad_x"][3] == 0).all()
    assert not failures, name + ": " + "; ".join(failures)


def test_fp64_matvec_restatement_meets_the_reference():
    fx = load_fixture()
    x, w = (torch.from_numpy(fx[k]).double().requires_grad_(True) for k in ("x", "weight"))
    out, mx = mobius_matvec_ref(w, x)
    gx, gw = torch.autograd.grad(out, [x, w], torch.from_numpy(fx["grad_output"]).double())
    failures = []
    _meets("out", out, fx["matvec.out"], failures)
    _meets("grad_x", gx, fx["matvec.grad_x"], failures)
    _meets("grad_weight", gw, fx["matvec.grad_weight"], failures)
    assert not failures, "; ".join(failures)
    assert bool((out[3] == 0).all()) and (fx["matvec.out"][3] == 0).all() and bool((gx[3] == 0).all())
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())


def test_header_and_binding_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", body))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
    assert "#define HYPAD_ABI_VERSION 7" in header
    for const in ("HYPAD_ML_HYPER_INPUT = 1", "HYPAD_ML_HYPER_BIAS = 2", "HYPAD_NONLIN_NONE = 0", "HYPAD_NONLIN_TANH = 1", "HYPAD_NONLIN_RELU = 2"):
        assert const in body, const
    from hypad_amd import _C
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and hasattr(_C.lib, name), name
    assert (_C.ML_HYPER_INPUT, _C.ML_HYPER_BIAS, _C.NONLIN_NONE, _C.NONLIN_TANH, _C.NONLIN_RELU) == (1, 2, 0, 1, 2)


def test_mobius_linear_module_takes_the_flags_and_keeps_its_state_dict():
    """A hyperbolic bias is a ManifoldParameter on the ball, a Euclidean one stays a plain nn.Parameter, bias=False leaves None; the
    state_dict keys are nn.Linear's in every case.  (Construction needs no GPU.)"""
    from hypad_amd.hyperspace import hyrnn_nets
    ball = hyrnn_nets.MobiusLinear(7, 5, fp64_hyper=False)
    assert ball.hyperbolic_input and ball.hyperbolic_bias and ball.nonlin is None
    assert isinstance(ball.bias, hyrnn_nets.ManifoldParameter) and float(ball.bias.norm()) < 1
    eucl = hyrnn_nets.MobiusLinear(7, 5, hyperbolic_input=False, hyperbolic_bias=False, nonlin=torch.relu, fp64_hyper=False)
    assert type(eucl.bias) is torch.nn.Parameter and eucl.nonlin is torch.relu and not eucl.hyperbolic_input
    none = hyrnn_nets.MobiusLinear(7, 5, bias=False, nonlin=torch.tanh, fp64_hyper=False)
    assert none.bias is None
    assert list(ball.state_dict()) == list(eucl.state_dict()) == ["weight", "bias"] and list(none.state_dict()) == ["weight"]
    with pytest.raises(NotImplementedError, match="supported"):
        hyrnn_nets.MobiusLinear(7, 5)                      # fp64_hyper=True, the reference's default
