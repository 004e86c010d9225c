"""The Moebius GRU on the host: the plain-torch restatement of tests/mobius_gru_ref.py against tests/golden/mobius_gru.npz -- the outputs
and gradients of the reference's own ``mobius_gru_cell``, ``mobius_gru_loop`` and ``mobius_pointwise_mul`` at k = -1 in fp32
(tests/golden/gen_mobius_gru.py) -- which it meets in fp64 and in fp32 at 1e-6 (error relative to max(1, max|recorded|), as
sweep_common.rel_err); the C ABI's new entry points; the workspace size; the refusals of the Python functions, which raise before anything
touches a device.
"""
import os
import re

import numpy as np
import pytest
import torch

import sweep_common as sc
from mobius_gru_ref import NONLINS, gru_cell_ref, gru_loop_ref, gru_packed_ref, pointwise_mul_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "mobius_gru.npz")
B, I, H, T = 9, 7, 5, 4
BATCH_SIZES = [9, 7, 7, 4]
PARAMS = ("weight_ih", "weight_hh", "bias")
NEW_ENTRY_POINTS = ("hypad_mobius_pointwise_mul_fwd", "hypad_mobius_pointwise_mul_bwd", "hypad_mobius_gru_workspace_bytes", "hypad_mobius_gru_fwd",
                    "hypad_mobius_gru_bwd")


def load_fixture():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def _leaves(fx, names, dt):
    return [torch.from_numpy(fx[n]).to(dt).requires_grad_(True) for n in names]


def _meets(what, got, recorded, failures, tol=1e-6):
    err, i = sc.rel_err(got, recorded)
    if not err <= tol:
        failures.append(f"{what}: {err:.3e} > {tol:g} at flat index {i}")


def _compare(fx, case, tag, arrays, failures):
    assert set(arrays) == {k.split(".", 1)[1] for k in fx if k.startswith(case + ".")}, case
    for name, t in arrays.items():
        _meets(f"{tag} {case}.{name}", t, fx[f"{case}.{name}"], failures)


def test_fixture_holds_every_case():
    fx = load_fixture()
    assert fx["x"].shape == (T, B, I) and fx["h0"].shape == (B, H) and fx["weight_ih"].shape == (3 * H, I) and fx["weight_hh"].shape == (3 * H, H)
    assert fx["bias"].shape == (3, H) and fx["x_packed"].shape == (sum(BATCH_SIZES), I)
    assert (fx["x"][0, 3] == 0).all() and (fx["h0"][6] == 0).all() and abs(np.linalg.norm(fx["h0"][2].astype(np.float64)) - 0.9) < 1e-6
    for k in ("x", "h0", "x_packed", "bias", "pmul_x"):
        assert np.linalg.norm(fx[k].astype(np.float64), axis=-1).max() < 0.91, k
    assert (np.abs(fx["pmul_w"][4] * fx["pmul_x"][4]) <= 1e-8).all() and (fx["pmul.out"][4] == 0).all() and (fx["pmul.out"][3] != 0).any()
    cases = ["cell_none", "cell_tanh", "cell_relu", "loop_ball", "loop_default", "packed", "pmul"]
    assert {k.split(".")[0] for k in fx if "." in k} == set(cases)
    assert len(fx) == 14 + 3 * 6 + 3 * 7 + 3
    for k, v in fx.items():
        assert v.dtype == np.float32 and np.isfinite(v).all(), k
    # what the loop records is the cell applied T times; the non-linearities differ
    assert np.allclose(fx["loop_ball.outs"][0], fx["cell_none.out"], rtol=0, atol=1e-6) and (fx["loop_ball.h_last"] == fx["loop_ball.outs"][-1]).all()
    assert not np.allclose(fx["cell_none.out"], fx["cell_tanh.out"], atol=1e-4) and not np.allclose(fx["cell_tanh.out"], fx["cell_relu.out"], atol=1e-4)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_reference(dt):
    fx, failures = load_fixture(), []
    tag = "fp64" if dt == torch.float64 else "fp32"
    G = lambda n: torch.from_numpy(fx[n]).to(dt)
    for name, fn in NONLINS.items():
        x, h, w_ih, w_hh, b = _leaves(fx, ("x", "h0") + PARAMS, dt)
        o = gru_cell_ref(x[0], h, w_ih, w_hh, b, fn)
        gs = torch.autograd.grad(o, [x, h, w_ih, w_hh, b], G("grad_cell"))
        _compare(fx, f"cell_{name}", tag, dict(out=o, grad_x=gs[0][0], grad_h=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4]), failures)
    for case, xn, hn, hyper in (("loop_ball", "x", "h0", True), ("loop_default", "x_tangent", "h0_tangent", False)):
        x, h, w_ih, w_hh, b = _leaves(fx, (xn, hn) + PARAMS, dt)
        outs, hl, _ = gru_loop_ref(x, h, w_ih, w_hh, b, None, hyper, hyper)
        gs = torch.autograd.grad(outs, [x, h, w_ih, w_hh, b], G("grad_outs"))
        _compare(fx, case, tag, dict(outs=outs, h_last=hl, grad_x=gs[0], grad_h0=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4]),
                 failures)
    x, h, w_ih, w_hh, b = _leaves(fx, ("x_packed", "h0") + PARAMS, dt)
    outs, hl, _ = gru_packed_ref(x, h, w_ih, w_hh, b, BATCH_SIZES, torch.tanh)
    gs = torch.autograd.grad([outs, hl], [x, h, w_ih, w_hh, b], [G("grad_packed"), G("grad_h_last")])
    _compare(fx, "packed", tag, dict(outs=outs, h_last=hl, grad_x=gs[0], grad_h0=gs[1], grad_weight_ih=gs[2], grad_weight_hh=gs[3], grad_bias=gs[4]),
             failures)
    w, x = _leaves(fx, ("pmul_w", "pmul_x"), dt)
    o = pointwise_mul_ref(w, x)
    gs = torch.autograd.grad(o, [w, x], G("grad_cell"))
    _compare(fx, "pmul", tag, dict(out=o, grad_w=gs[0], grad_x=gs[1]), failures)
    assert not failures, "; ".join(failures)


def test_header_and_binding_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", body))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, name
    assert "#define HYPAD_ABI_VERSION 7" in header
    for cite in ("math_.py:1361-1371", "hyperspace/hyrnn_nets.py:61-151"):
        assert cite in header, cite
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and hasattr(_C.lib, name), name
    assert declared == set(_C.EXPORTS)
    from hypad_amd import build
    assert "mobius_gru.hip" in build.SOURCES


def test_workspace_size_is_a_function_of_the_shape_alone():
    from hypad_amd import _C
    for steps, rows, i, h in ((1, 17, 33, 63), (5, 39, 100, 100), (2, 4099, 100, 100), (3, 0, 7, 5)):
        # x W_ih^T / its gradient (3H), g_mh_r, g_mh_z, g_mrh, rh, h_prev (H each), the per-row bias gradients (3H), the dense backward's
        # scratch (3H) and dL/d|x| (1) per (step, row)
        assert _C.lib.hypad_mobius_gru_workspace_bytes(steps, rows, i, h) == 4 * steps * rows * (14 * h + 1), (steps, rows, i, h)
    assert _C.lib.hypad_mobius_gru_workspace_bytes(0, 4, 7, 5) == 0 and _C.lib.hypad_mobius_gru_workspace_bytes(2, -1, 7, 5) == 0


def test_refusals_raise_before_touching_a_device():
    from hypad_amd.hyperspace import gmath, hyrnn_nets
    x, h = torch.zeros(4, 9, 7), torch.zeros(9, 5)                         # host tensors: a device call would raise HypadError
    w_ih, w_hh, b = torch.zeros(15, 7), torch.zeros(15, 5), torch.zeros(3, 5)
    cell, loop = hyrnn_nets.mobius_gru_cell, hyrnn_nets.mobius_gru_loop
    for call in (lambda: cell(x[0], h, w_ih, w_hh, b, 1.0),
                 lambda: cell(x[0], h, w_ih, w_hh, b, torch.tensor(-0.5)),
                 lambda: cell(x[0], h, w_ih, w_hh, b, -1.0, nonlin=torch.sigmoid),
                 lambda: cell(x[0], h, w_ih, w_hh, b, -1.0, nonlin=lambda t: t),
                 lambda: cell(x[0], h, w_ih[:14], w_hh, b, -1.0),
                 lambda: cell(x[0], h, w_ih, w_hh.t(), b, -1.0),
                 lambda: cell(x[0], h, w_ih, w_hh, b.reshape(-1), -1.0),
                 lambda: cell(x[0, :8], h, w_ih, w_hh, b, -1.0),
                 lambda: cell(x, h, w_ih, w_hh, b, -1.0),
                 lambda: cell(torch.zeros(9, 257), h, torch.zeros(15, 257), w_hh, b, -1.0),
                 lambda: cell(x[0], torch.zeros(9, 257), torch.zeros(771, 7), torch.zeros(771, 257), torch.zeros(3, 257), -1.0),
                 lambda: loop(x, h, w_ih, w_hh, b, 1.0),
                 lambda: loop(x, h, w_ih, w_hh, b, -1.0, nonlin=torch.sigmoid),
                 lambda: loop(x[:, :8], h, w_ih, w_hh, b, -1.0),
                 lambda: loop(x[0], h, w_ih, w_hh, b, -1.0),
                 lambda: loop(x, h, w_ih, w_hh[:, :4], b, -1.0),
                 lambda: loop(torch.zeros(27, 7), h, w_ih, w_hh, b, -1.0, batch_sizes=[9, 7, 7, 3]),
                 lambda: loop(torch.zeros(27, 7), h, w_ih, w_hh, b, -1.0, batch_sizes=[8, 8, 7, 4]),
                 lambda: loop(torch.zeros(27, 7), h, w_ih, w_hh, b, -1.0, batch_sizes=[9, 4, 7, 7]),
                 lambda: loop(x, h, w_ih, w_hh, b, -1.0, batch_sizes=[9, 7, 7, 4]),
                 lambda: hyrnn_nets.one_rnn_transform(w_hh[:5], h, w_ih[:5], x[0], b[0], 1.0),
                 lambda: gmath.mobius_pointwise_mul(h, h, k=1.0),
                 lambda: gmath.mobius_pointwise_mul(h, h, k=-1.0, dim=0),
                 lambda: gmath.mobius_pointwise_mul(h[:4], h, k=-1.0),
                 lambda: gmath.mobius_pointwise_mul(torch.zeros(9, 4), h, k=-1.0),
                 lambda: gmath.mobius_pointwise_mul(torch.zeros(9, 257), torch.zeros(9, 257), k=-1.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            call()
    # the same signatures and defaults as the reference's functions (hyperspace/hyrnn_nets.py:61-105)
    import inspect
    assert list(inspect.signature(hyrnn_nets.one_rnn_transform).parameters) == ["W", "h", "U", "x", "b", "k"]
    assert list(inspect.signature(cell).parameters) == ["input", "hx", "weight_ih", "weight_hh", "bias", "k", "nonlin"]
    sig = inspect.signature(loop).parameters
    assert list(sig) == ["input", "h0", "weight_ih", "weight_hh", "bias", "k", "batch_sizes", "hyperbolic_input", "hyperbolic_hidden_state0", "nonlin"]
    assert [sig[n].default for n in ("batch_sizes", "hyperbolic_input", "hyperbolic_hidden_state0", "nonlin")] == [None, False, False, None]
    assert inspect.signature(cell).parameters["nonlin"].default is None
