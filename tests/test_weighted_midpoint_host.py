"""The weighted Moebius gyromidpoint and mobius_scalar_mul on the host: the restatement of tests/midpoint_ref.py against the
reference's own recorded outputs (tests/golden/weighted_midpoint.npz, written by tests/golden/gen_weighted_midpoint.py), the C ABI's
declarations and bindings, and the refusals of the Python functions -- which come before any device call, so they run here.

The bound.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative
to max(1, max|array|) (measured worst: 1.3e-7); the restatement is held to the fp32 records at the same 1e-6, run in fp64 and in fp32.
One row is held to nothing in fp64: grad_x of mobius_scalar_mul's all-zero row, where the reference itself returns 0 in fp32 and
r g in fp64 (the generator's docstring).
"""
import os
import re

import numpy as np
import pytest
import torch

from midpoint_ref import mobius_scalar_mul_ref, weighted_midpoint_bmm_ref, weighted_midpoint_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6
SMUL_ZERO_ROW = 3
BMM_KINDS = ("softmax", "signed", "zerow")
# name: (reducedim, keepdim, weights, posweight, lincomb, coadd) -- the generator's table
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
NEW_ENTRY_POINTS = ("hypad_mobius_scalar_mul_fwd", "hypad_mobius_scalar_mul_bwd", "hypad_weighted_midpoint_workspace_bytes",
                    "hypad_weighted_midpoint_fwd", "hypad_weighted_midpoint_bwd", "hypad_weighted_midpoint_bmm_workspace_bytes",
                    "hypad_weighted_midpoint_bmm_fwd", "hypad_weighted_midpoint_bmm_bwd")


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "weighted_midpoint.npz")) as z:
        return {k: z[k] for k in z.files}


def bmm_name(kind, lincomb):
    return f"bmm_{kind}_lincomb{int(lincomb)}"


def _leaf(a, dt):
    return None if a is None else torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True)


def _meets(fx, name, labels, fn, operands, go, dt, skip=None):
    leaves = [_leaf(a, dt) for a in operands]
    o = fn(*leaves)
    rec = fx[f"{name}.out"]
    assert tuple(o.shape) == rec.shape, (name, tuple(o.shape), rec.shape)
    gs = torch.autograd.grad(o, [t for t in leaves if t is not None], torch.from_numpy(go.astype(np.float64)).to(dt).reshape(o.shape))
    for lab, got in zip(labels, [o.detach()] + list(gs)):
        rec = fx[f"{name}.{lab}"].astype(np.float64)
        d = np.abs(got.double().numpy().reshape(rec.shape) - rec)
        if skip and skip[0] == lab:
            d[skip[1]] = 0
        err = float(d.max()) / max(1.0, float(np.abs(rec).max()))
        assert err <= BOUND, (name, lab, str(dt), err)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_recorded_reference(dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 for v in fx.values())
    for kind in BMM_KINDS:
        for lincomb in (False, True):
            _meets(fx, bmm_name(kind, lincomb), ("out", "grad_xs", "grad_w"), lambda x, w, lc=lincomb: weighted_midpoint_bmm_ref(x, w, lincomb=lc),
                   (fx["bmm_xs"], fx[f"bmm_w_{kind}"]), fx["bmm_grad_output"], dt)
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in REDUCE_CASES.items():
        fn = lambda x, w=None: weighted_midpoint_ref(x, w, reducedim=reducedim, keepdim=keepdim, lincomb=lincomb, posweight=posweight, coadd=coadd)
        _meets(fx, "red_" + name, ("out", "grad_xs") + (() if wk is None else ("grad_w",)), lambda x, w: fn(x, w),
               (fx["red_xs"], None if wk is None else fx[f"red_w_{wk}"]), fx["red_grad_output_all" if reducedim is None else "red_grad_output_r0"], dt)
    for name, r in (("smul_rows", fx["smul_r_rows"]), ("smul_scalar", fx["smul_r_scalar"])):
        _meets(fx, name, ("out", "grad_r", "grad_x"), mobius_scalar_mul_ref, (r, fx["smul_x"]), fx["smul_grad_output"], dt,
               skip=("grad_x", SMUL_ZERO_ROW) if dt == torch.float64 else None)


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    assert fx["bmm_xs"].shape == (2, 7, 3) and fx["bmm_w_softmax"].shape == (2, 5, 7) and fx["red_xs"].shape == (6, 9, 5)
    assert not fx["bmm_xs"][0, 2].any() and abs(float(np.linalg.norm(fx["bmm_xs"][1, 4])) - 0.9) < 1e-6
    assert not fx["bmm_w_zerow"][1, 3].any() and not fx["bmm_zerow_lincomb0.out"][1, 3].any() and not fx["smul_x"][SMUL_ZERO_ROW].any()
    assert (fx["bmm_w_signed"] < 0).any() and (fx["red_w_signed"] < 0).any() and (fx["red_w_pos"] > 0).all()
    assert np.allclose(fx["bmm_w_softmax"].sum(-1), 1.0, atol=1e-6)
    assert fx["red_all_pos.out"].shape == (5,) and fx["red_r0_pos_keepdim.out"].shape == (1, 9, 5) and fx["red_r0_pos.out"].shape == (9, 5)
    assert all(np.isfinite(v).all() for v in fx.values())


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert re.search(r"#define HYPAD_ABI_VERSION 7\b", text)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b(int|size_t) " + name + r"\(", text), name
    assert re.search(r"HYPAD_MID_LINCOMB = 1, HYPAD_MID_POSWEIGHT = 2, HYPAD_MID_COADD = 4", text)
    for cite in ("math_.py:788-858", "math_.py:1953-2087", "math_.py:2090-2122"):
        assert cite in text, cite
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes is not None, name
    assert (_C.MID_LINCOMB, _C.MID_POSWEIGHT, _C.MID_COADD) == (1, 2, 4)


def test_midpoint_source_is_built_into_the_library():
    from hypad_amd import build
    assert "midpoint.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "midpoint.hip"))


def test_python_functions_refuse_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd.hyperspace import gmath
    x, w = torch.zeros(2, 7, 3), torch.zeros(2, 5, 7)
    for bad in (dict(k=-0.5), dict(k=1.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.weighted_midpoint_bmm(x, w, **bad)
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.weighted_midpoint(x, bad["k"])
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.mobius_scalar_mul(torch.tensor(2.0), x, k=bad["k"])
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.weighted_midpoint(x, -1.0, dim=1)
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.mobius_scalar_mul(torch.tensor(2.0), x, k=-1.0, dim=0)
    wide = torch.zeros(2, 7, 257)
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.weighted_midpoint_bmm(wide, w, -1.0)
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.weighted_midpoint(wide, -1.0)
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.mobius_scalar_mul(torch.tensor(2.0), wide, k=-1.0)
    for xs_, w_ in ((x, torch.zeros(2, 5, 8)), (x, torch.zeros(3, 5, 7)), (torch.zeros(4, 2, 7, 3), torch.zeros(2, 5, 7)), (torch.zeros(3), w),
                    (x.double(), w)):
        with pytest.raises(NotImplementedError, match="supported"):              # mismatched shapes, batch dimensions, dtype
            gmath.weighted_midpoint_bmm(xs_, w_, -1.0)
    for w_ in (torch.zeros(2, 6), torch.zeros(7, 2), torch.zeros(2, 7, 3), torch.zeros(3, 2, 7)):
        with pytest.raises(NotImplementedError, match="supported"):              # weights that do not broadcast against xs.shape[:-1]
            gmath.weighted_midpoint(x, -1.0, weights=w_)
    for rd in ([2], [0, 0], [-1], [5]):
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.weighted_midpoint(x, -1.0, reducedim=rd)
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.mobius_scalar_mul(torch.zeros(2, 7), x, k=-1.0)                  # r is neither one value nor x.shape[:-1] + (1,)
    # what is supported gets as far as the device and is refused there, on a host without one
    from hypad_amd import _C
    for call in (lambda: gmath.weighted_midpoint_bmm(x, w, -1.0), lambda: gmath.weighted_midpoint(x, -1.0, weights=torch.zeros(7)),
                 lambda: gmath.weighted_midpoint(x, -1.0, reducedim=[-2], keepdim=True), lambda: gmath.mobius_scalar_mul(torch.zeros(2, 7, 1), x, k=-1.0)):
        with pytest.raises(_C.HypadError, match="GPU"):
            call()
