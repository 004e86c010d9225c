"""The geodesic distances dist_matmul, dist and dist0 on the host: the restatement of tests/dist_ref.py against the reference's own
recorded outputs (tests/golden/dist.npz, written by tests/golden/gen_dist.py), the C ABI's declarations and bindings, and the refusals
of the Python functions -- which come before any device call, so they run here.

The bound.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative
to max(1, max|array|) (measured worst: 2.2e-7, dm.out); the restatement is held to the fp32 records at the same 1e-6, run in fp64 and
in fp32.
"""
import os
import re

import numpy as np
import pytest
import torch

from dist_ref import dist0_ref, dist_matmul_ref, dist_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 1e-6
# the generator's named cases
PAIR_RIM_X, PAIR_ZERO_X, PAIR_ZERO_Y = (1, 3), (0, 2), (0, 4)
ROW_ZERO_X, ROW_ZERO_Y, ROW_ZERO_BOTH, ROW_EQUAL, ROW_RIM = 1, 2, 3, 4, 5
NEW_ENTRY_POINTS = ("hypad_dist_matmul_fwd", "hypad_dist_matmul_bwd", "hypad_dist_fwd", "hypad_dist_bwd", "hypad_dist0_fwd", "hypad_dist0_bwd")
# name: (labels, function of the leaves, operand keys, grad_output key)
CASES = {
    "dm": (("out", "grad_x", "grad_y"), dist_matmul_ref, ("dm_x", "dm_y"), "dm_grad_output"),
    "dist": (("out", "grad_x", "grad_y"), dist_ref, ("row_x", "row_y"), "row_grad_output"),
    "dist0": (("out", "grad_x"), dist0_ref, ("row_x",), "row_grad_output"),
}


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "dist.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_recorded_reference(dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 for v in fx.values())
    for name, (labels, fn, keys, gokey) in CASES.items():
        leaves = [torch.from_numpy(fx[k].astype(np.float64)).to(dt).requires_grad_(True) for k in keys]
        o = fn(*leaves)
        assert tuple(o.shape) == fx[f"{name}.out"].shape, (name, tuple(o.shape))
        gs = torch.autograd.grad(o, leaves, torch.from_numpy(fx[gokey].astype(np.float64)).to(dt))
        for lab, got in zip(labels, [o.detach()] + list(gs)):
            rec = fx[f"{name}.{lab}"].astype(np.float64)
            err = float(np.abs(got.double().numpy() - rec).max()) / max(1.0, float(np.abs(rec).max()))
            assert err <= BOUND, (name, lab, str(dt), err)


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    x, y = fx["dm_x"], fx["dm_y"]
    assert x.shape == (2, 5, 3) and y.shape == (2, 3, 7) and fx["dm.out"].shape == (2, 5, 7) and fx["dm.grad_y"].shape == (2, 3, 7)
    assert abs(float(np.linalg.norm(x[PAIR_RIM_X])) - 0.9) < 1e-6 and not x[PAIR_ZERO_X].any() and not y[PAIR_ZERO_Y[0], :, PAIR_ZERO_Y[1]].any()
    assert PAIR_ZERO_X[0] == PAIR_ZERO_Y[0]
    at = (PAIR_ZERO_X[0], PAIR_ZERO_X[1], PAIR_ZERO_Y[1])
    assert 0.0 <= float(fx["dm.out"][at]) <= 2.02 * np.arctanh(np.sqrt(1e-15))
    sep = np.linalg.norm(x[:, :, None, :].astype(np.float64) - np.swapaxes(y, -1, -2)[:, None, :, :], axis=-1)
    sep[at] = np.inf
    assert float(sep.min()) >= 0.05
    assert float(np.linalg.norm(x.reshape(-1, 3), axis=1).max()) <= 0.9 + 1e-6 and float(np.linalg.norm(np.swapaxes(y, -1, -2), axis=-1).max()) <= 0.8
    rx, ry = fx["row_x"], fx["row_y"]
    assert rx.shape == ry.shape == (9, 5) and fx["dist.out"].shape == fx["dist0.out"].shape == (9,)
    assert not rx[ROW_ZERO_X].any() and ry[ROW_ZERO_X].any() and not ry[ROW_ZERO_Y].any() and rx[ROW_ZERO_Y].any()
    assert not rx[ROW_ZERO_BOTH].any() and not ry[ROW_ZERO_BOTH].any()
    assert np.array_equal(rx[ROW_EQUAL], ry[ROW_EQUAL]) and rx[ROW_EQUAL].any() and abs(float(np.linalg.norm(rx[ROW_RIM])) - 0.9) < 1e-6
    for row in (ROW_EQUAL, ROW_ZERO_BOTH):                 # distance 0 and gradient 0, from the reference itself
        assert fx["dist.out"][row] == 0 and not fx["dist.grad_x"][row].any() and not fx["dist.grad_y"][row].any()
    assert fx["dist0.out"][ROW_ZERO_X] == 0 and not fx["dist0.grad_x"][ROW_ZERO_X].any() and not fx["dist0.grad_x"][ROW_ZERO_BOTH].any()
    assert all(np.isfinite(v).all() for v in fx.values())


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert re.search(r"#define HYPAD_ABI_VERSION 7\b", text)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint " + name + r"\(", text), name
    for cite in ("math_.py:905-947", "math_.py:861-902", "math_.py:950-975"):
        assert cite in text, cite
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    for name in NEW_ENTRY_POINTS:
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes is not None, name
    assert len(_C._SIGS["hypad_dist_matmul_fwd"][1]) == 8 and len(_C._SIGS["hypad_dist_matmul_bwd"][1]) == 10
    assert len(_C._SIGS["hypad_dist_fwd"][1]) == 6 and len(_C._SIGS["hypad_dist_bwd"][1]) == 8
    assert len(_C._SIGS["hypad_dist0_fwd"][1]) == 5 and len(_C._SIGS["hypad_dist0_bwd"][1]) == 6


def test_dist_source_is_built_into_the_library():
    from hypad_amd import build
    assert "dist.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "dist.hip"))


def test_python_functions_refuse_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    x, y, r = torch.zeros(2, 5, 3), torch.zeros(2, 3, 7), torch.zeros(9, 5)
    for k in (-0.5, 1.0, 0.0):
        for call in (lambda: gmath.dist_matmul(x, y, k), lambda: gmath.dist(r, r, k=k), lambda: gmath.dist0(r, k=k)):
            with pytest.raises(NotImplementedError, match="supported"):
                call()
    for call in (lambda: gmath.dist(r, r, k=-1.0, dim=0), lambda: gmath.dist0(r, k=-1.0, dim=0), lambda: gmath.dist0(torch.zeros(()), k=-1.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            call()
    wide = torch.zeros(2, 257)
    for call in (lambda: gmath.dist_matmul(torch.zeros(2, 5, 257), torch.zeros(2, 257, 7), -1.0), lambda: gmath.dist(wide, wide, k=-1.0),
                 lambda: gmath.dist0(wide, k=-1.0), lambda: gmath.dist0(r.double(), k=-1.0), lambda: gmath.dist(r.double(), r.double(), k=-1.0),
                 lambda: gmath.dist(r, r.double(), k=-1.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            call()
    # operands that do not fit: the contraction, the batch dimensions, the dtype, too few dimensions, 2^31 distances
    for x_, y_ in ((x, torch.zeros(2, 4, 7)), (x, torch.zeros(3, 3, 7)), (torch.zeros(4, 2, 5, 3), torch.zeros(2, 3, 7)), (torch.zeros(3), y),
                   (x, torch.zeros(3)), (x.double(), y), (x, y.double()), (torch.zeros(2, 5, 0), torch.zeros(2, 0, 7)),
                   (torch.zeros(1, 1).expand(65536, 1), torch.zeros(1, 1).expand(1, 32768))):
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.dist_matmul(x_, y_, -1.0)
    for y_ in (torch.zeros(5), torch.zeros(1, 5), torch.zeros(9, 4), torch.zeros(9, 5, 1)):
        with pytest.raises(NotImplementedError, match="supported"):              # nothing is broadcast
            gmath.dist(r, y_, k=-1.0)
    # what is supported gets as far as the device and is refused there, on a host without one
    for call in (lambda: gmath.dist_matmul(x, y, -1.0), lambda: gmath.dist_matmul(x[0], y, -1.0), lambda: gmath.dist_matmul(x, y[0], -1.0),
                 lambda: gmath.dist_matmul(x, torch.zeros(2, 7, 3).transpose(-1, -2), torch.tensor(-1.0)), lambda: gmath.dist(r, r, k=-1.0),
                 lambda: gmath.dist(r, r, k=-1.0, keepdim=True, dim=1), lambda: gmath.dist0(r, k=-1.0), lambda: gmath.dist0(x, k=None, dim=2)):
        with pytest.raises(_C.HypadError, match="GPU"):
            call()
