"""dist2plane_matmul on the host: the restatement of tests/dist2plane_matmul_ref.py against the reference's own recorded outputs
(tests/golden/dist2plane_matmul.npz, written by tests/golden/gen_dist2plane_matmul.py), its hand-written backward against autograd, the
identities the GPU test asks of the library, the C ABI's declarations, bindings and size checks, and the refusals of the Python function
-- which come before any device call, so they run here.

The bounds.  fp64 against fp64: 1e-12, the project's figure, relative to max(1, max|array|).  The fp32 restatement against the fp32
record: 8 * own + 2e-6 (the constants of sweep_common.Ck), own = the reference's fp32 run against its own fp64 run on that array, which
the generator printed -- out 3.24e-07, grad_x 3.78e-08, grad_p 2.76e-08, grad_z 5.21e-09 -- and which is recomputed here from the two
records.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from dist2plane_matmul_ref import dist2plane_matmul_bwd, dist2plane_matmul_ref
from dist2plane_ref import dist2plane_ref
from test_tangent_maps_host import _header_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
FP64_BOUND = 1e-12
CK_C, CK_F = 8.0, 2e-6
PRINTED_OWN = {"out": 3.24e-07, "grad_x": 3.78e-08, "grad_p": 2.76e-08, "grad_z": 5.21e-09}
LABELS = ("out", "grad_x", "grad_p", "grad_z")
ZERO_X, ZERO_P, ZERO_Z, EQUAL_X, EQUAL_P = (0, 2), (0, 4), (1, 3), (1, 1), (1, 5)      # the generator's named cases
NEW_ENTRY_POINTS = ("hypad_dist2plane_matmul_fwd", "hypad_dist2plane_matmul_bwd")
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                              # include/hypad.h


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "dist2plane_matmul.npz")) as z:
        return {k: z[k] for k in z.files}


def _err(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) / max(1.0, float(np.abs(want).max()))


def _restated(fx, dt):
    leaves = [torch.from_numpy(fx[k].astype(np.float64)).to(dt).requires_grad_(True) for k in ("x", "p", "z")]
    o = dist2plane_matmul_ref(*leaves)
    gs = torch.autograd.grad(o, leaves, torch.from_numpy(fx["grad_output"].astype(np.float64)).to(dt))
    return [o.detach().numpy()] + [g.numpy() for g in gs]


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    x, p, z = fx["x"], fx["p"], fx["z"]
    assert x.shape == (2, 5, 3) and p.shape == z.shape == (2, 3, 7) and fx["grad_output"].shape == (2, 5, 7)
    assert all(fx[k].dtype == np.float32 for k in ("x", "p", "z", "grad_output"))
    for lab, shape in zip(LABELS, ((2, 5, 7), (2, 5, 3), (2, 3, 7), (2, 3, 7))):
        assert fx[f"d2pm.{lab}"].shape == fx[f"d2pm64.{lab}"].shape == shape
        assert fx[f"d2pm.{lab}"].dtype == np.float32 and fx[f"d2pm64.{lab}"].dtype == np.float64
    assert len(fx) == 12 and all(np.isfinite(v).all() for v in fx.values())
    assert not x[ZERO_X].any() and not p[ZERO_P[0], :, ZERO_P[1]].any() and not z[ZERO_Z[0], :, ZERO_Z[1]].any()
    assert np.array_equal(x[EQUAL_X], p[EQUAL_P[0], :, EQUAL_P[1]]) and x[EQUAL_X].any()
    assert float(np.linalg.norm(x.astype(np.float64), axis=-1).max()) <= 0.6 + 1e-6
    assert float(np.linalg.norm(p.astype(np.float64), axis=-2).max()) <= 0.6 + 1e-6
    zn = np.linalg.norm(z.astype(np.float64), axis=-2)
    live = np.ones_like(zn, dtype=bool)
    live[ZERO_Z] = False
    assert float(zn[live].min()) >= 0.3 - 1e-6 and float(zn.max()) <= 2.0 + 1e-6
    for rec in ("d2pm", "d2pm64"):                          # the zero normal, from the reference itself
        b, j = ZERO_Z
        assert not fx[rec + ".out"][b, :, j].any() and not fx[rec + ".grad_p"][b, :, j].any() and not fx[rec + ".grad_z"][b, :, j].any()
    for lab in LABELS:                                      # what the generator printed
        own = _err(fx[f"d2pm.{lab}"], fx[f"d2pm64.{lab}"])
        assert abs(own - PRINTED_OWN[lab]) <= 0.01 * PRINTED_OWN[lab], (lab, own)


def test_restatement_in_fp64_meets_the_fp64_record():
    fx = load_fixture()
    for lab, got in zip(LABELS, _restated(fx, F64)):
        err = _err(got, fx[f"d2pm64.{lab}"])
        assert err <= FP64_BOUND, (lab, err)


def test_restatement_in_fp32_meets_the_fp32_record():
    fx = load_fixture()
    for lab, got in zip(LABELS, _restated(fx, torch.float32)):
        own = _err(fx[f"d2pm.{lab}"], fx[f"d2pm64.{lab}"])
        err = _err(got, fx[f"d2pm.{lab}"])
        assert err <= CK_C * own + CK_F, (lab, err, own)


# ------------------------------------------------------------------------------------------------ the hand backward, the identities
def _data(batch, N, M, D, seed, special=False):
    """fp64 copies of fp32 operands: points within radius 0.6, normals N(0, 1) at norms in [0.3, 2], g ~ N(0, 1) / numel; special: an
    all-zero x row, p column and z column, and (from two rows and two planes on) an x row equal to a p column."""
    g = torch.Generator().manual_seed(seed)

    def ball(rows):
        a = torch.randn(batch, rows, D, generator=g, dtype=F64)
        return a / a.norm(dim=-1, keepdim=True) * (0.05 + 0.55 * torch.rand(batch, rows, 1, generator=g, dtype=F64))

    x, pp = ball(N), ball(M)
    zz = torch.randn(batch, M, D, generator=g, dtype=F64)
    zz = zz / zz.norm(dim=-1, keepdim=True) * (0.3 + 1.7 * torch.rand(batch, M, 1, generator=g, dtype=F64))
    if special:
        x[0, 0] = 0.0
        pp[0, 1 % M] = 0.0
        zz[0, 2 % M] = 0.0
        if N >= 2 and M >= 4:
            x[-1, 1] = pp[-1, 3]
    go = torch.randn(batch, N, M, generator=g, dtype=F64) / (batch * N * M)
    f = lambda t: t.float().double()
    return f(x), f(pp).transpose(-1, -2).contiguous(), f(zz).transpose(-1, -2).contiguous(), f(go)


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 9, 4, 1), (1, 3, 5, 64)], ids=lambda s: "x".join(map(str, s)))
def test_hand_written_backward_meets_autograd(shape):
    """Ordinary operands, and -- in a run of their own, so that their sizes do not set the scale for the others -- the special rows."""
    for special in (False, True):
        x, p, z, go = _data(*shape, seed=1000 * shape[1] + shape[3], special=special)
        leaves = [t.clone().requires_grad_(True) for t in (x, p, z)]
        want = torch.autograd.grad(dist2plane_matmul_ref(*leaves), leaves, go)
        got = dist2plane_matmul_bwd(x, p, z, go)
        for lab, a, b in zip(LABELS[1:], got, want):
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (lab, special)
            err = _err(a.numpy(), b.numpy())
            assert err <= FP64_BOUND, (lab, special, err)


def identities(fn, x, p, z, bwd=None):
    """[(name, left, right)] of the identities dist2plane_matmul satisfies, for ``fn(x, p, z)`` on operands of any dtype and device;
    tests/test_gpu_dist2plane_matmul.py asks the same of the library."""
    zn = z.norm(dim=-2, keepdim=True)
    zh = z / zn.clamp_min(1e-15)
    x0, p0 = torch.zeros_like(x), torch.zeros_like(p)
    d2p = torch.stack([dist2plane_ref(x0[b], p[b].t(), z[b].t(), signed=True, scaled=True) for b in range(x.shape[0])])
    out = fn(x, p, z)
    zz = z.clone()
    zz[..., 0] = 0.0
    res = [("x = 0 is twice dist2plane(signed, scaled)", fn(x0, p, z), 2 * d2p),
           ("p = 0", fn(x, p0, z), 2 * torch.asinh(2 * torch.matmul(x, zh)) * zn),
           ("odd in z", fn(x, p, -z), -out),
           ("homogeneous in z", fn(x, p, 2.5 * z), 2.5 * out),
           ("a zero normal", fn(x, p, zz)[..., 0], torch.zeros_like(out[..., 0]))]
    if bwd is not None:
        _, gp, gz = bwd(x, p, zz)
        res += [("a zero normal, grad_p", gp[..., 0], torch.zeros_like(gp[..., 0])), ("a zero normal, grad_z", gz[..., 0], torch.zeros_like(gz[..., 0]))]
    return res


@pytest.mark.parametrize("shape", [(1, 33, 9, 5), (2, 9, 20, 100)], ids=lambda s: "x".join(map(str, s)))
def test_restated_identities_hold_in_fp64(shape):
    x, p, z, go = _data(*shape, seed=7 * shape[1] + shape[3])

    def autograd_bwd(a, b, c):
        leaves = [t.clone().requires_grad_(True) for t in (a, b, c)]
        return torch.autograd.grad(dist2plane_matmul_ref(*leaves), leaves, go)

    for bwd in (autograd_bwd, lambda a, b, c: dist2plane_matmul_bwd(a, b, c, go)):
        for name, left, right in identities(dist2plane_matmul_ref, x, p, z, bwd):
            err = _err(left.numpy(), right.numpy())
            assert err <= FP64_BOUND, (name, err)
    # and it is not twice dist2plane away from x = 0
    d2p = torch.stack([dist2plane_ref(x[b], p[b].t(), z[b].t(), signed=True, scaled=True) for b in range(x.shape[0])])
    assert _err(dist2plane_matmul_ref(x, p, z).numpy(), (2 * d2p).numpy()) > 1e-2


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert "#define HYPAD_ABI_VERSION 7" in text and "math_.py:2125-2159" in text
    header = _header_signatures()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7          # new entry points, no changed one: the version stays
    for name in NEW_ENTRY_POINTS:
        assert name in header, name
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and args == header[name], (name, args, header[name])
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes == args, name
    assert len(_C._SIGS["hypad_dist2plane_matmul_fwd"][1]) == 9 and len(_C._SIGS["hypad_dist2plane_matmul_bwd"][1]) == 12
    assert not hasattr(_C.lib, "hypad_dist2plane_matmul_workspace_bytes")   # the fused walk needs no workspace


def test_the_source_is_built_into_the_library_last():
    from hypad_amd import build
    assert build.SOURCES[-1] == "dist2plane_matmul.hip" and build.SOURCES[-2] == "tangent.hip"
    text = open(os.path.join(build.CSRC, "dist2plane_matmul.hip")).read()
    assert all(f"int {name}(" in text for name in NEW_ENTRY_POINTS) and "asm" not in text and "atomic" not in text.replace("No atomics", "")


def test_entry_points_check_their_sizes_before_any_hip_call():
    """Host pointers throughout, on a machine that may have no device: every call below is answered by the argument checks, which come
    before the first HIP call of the entry point (anything later would return a HIP error code instead, or fault on the pointers)."""
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_float * 4096)()
    q, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    fwd = lambda ops=(q,) * 4, b=2, n=4, m=6, d=8: L.hypad_dist2plane_matmul_fwd(*ops, n64(b), n64(n), n64(m), d, None)
    bwd = lambda ops=(q,) * 4, gr=(q,) * 3, b=2, n=4, m=6, d=8: L.hypad_dist2plane_matmul_bwd(*ops, *gr, n64(b), n64(n), n64(m), d, None)
    for call in (fwd, bwd):
        assert call(d=257) == call(d=4096) == HYPAD_EUNSUPPORTED
        assert call(b=2 ** 20, n=2 ** 6, m=2 ** 5) == call(b=1, n=2 ** 16, m=2 ** 15) == HYPAD_EUNSUPPORTED       # 2^31 outputs
        assert call(b=1, n=2 ** 23, m=1, d=256) == call(b=2 ** 10, n=1, m=2 ** 13, d=256) == HYPAD_EUNSUPPORTED  # 2^31 elements of x; of p and z
        assert call(b=2 ** 31, n=0) == call(n=2 ** 31, m=0) == call(n=0, m=2 ** 31) == HYPAD_EUNSUPPORTED
        assert call(b=-1) == call(n=-1) == call(m=-2) == call(d=0) == call(d=-3) == HYPAD_EINVAL
        assert call(d=257, b=-1) == HYPAD_EINVAL
        for i in range(4):                                  # each operand (the last: out or grad_out) missing in turn
            assert call(ops=tuple(None if k == i else q for k in range(4))) == HYPAD_EINVAL, i
    # nothing to compute: nothing to launch, nothing to read (no gradient asked for, so nothing to zero either)
    assert fwd(ops=(None,) * 4, b=0) == 0 and fwd(ops=(None, q, q, None), n=0) == 0 and fwd(ops=(q, None, None, None), m=0) == 0
    none = (None,) * 3
    assert bwd(ops=(None,) * 4, gr=none, b=0) == 0 and bwd(ops=(None, q, q, None), gr=none, n=0) == 0 and bwd(ops=(q, None, None, None), gr=none, m=0) == 0
    assert fwd(ops=(None, q, q, q), m=0) == HYPAD_EINVAL and bwd(ops=(q, None, q, q), gr=none, n=0) == HYPAD_EINVAL      # rows that exist


def test_python_function_refuses_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    f = gmath.dist2plane_matmul
    x, p, z = torch.zeros(2, 5, 3), torch.zeros(2, 3, 7), torch.zeros(2, 3, 7)
    for k in (-0.5, 1.0, 0.0, torch.tensor(-2.0)):
        with pytest.raises(NotImplementedError, match="supported"):
            f(x, p, z, k=k)
    with pytest.raises(TypeError):
        f(x, p, z, -1.0)                                    # k is keyword-only, as in the reference
    bad = [(x, p, torch.zeros(2, 3, 6)), (x, p, torch.zeros(3, 7)), (x, torch.zeros(2, 4, 7), torch.zeros(2, 4, 7)),
           (x, torch.zeros(3, 3, 7), torch.zeros(3, 3, 7)), (torch.zeros(4, 2, 5, 3), p, z), (torch.zeros(3), p, z),
           (x, torch.zeros(3), torch.zeros(3)), (x.double(), p, z), (x, p.double(), z), (x, p, z.double()), (x.double(), p.double(), z.double()),
           (torch.zeros(2, 5, 0), torch.zeros(2, 0, 7), torch.zeros(2, 0, 7)), (torch.zeros(2, 5, 257), torch.zeros(2, 257, 7), torch.zeros(2, 257, 7)),
           (torch.zeros(1, 1).expand(65536, 1), torch.zeros(1, 1).expand(1, 32768), torch.zeros(1, 1).expand(1, 32768))]
    for x_, p_, z_ in bad:
        with pytest.raises(NotImplementedError, match="supported"):
            f(x_, p_, z_, k=-1.0)
    # what is supported gets as far as the device and is refused there, on host tensors
    pt = torch.zeros(2, 7, 3).transpose(-1, -2)
    for x_, p_, z_, k in ((x, p, z, -1.0), (x[0], p, z, -1.0), (x, p[0], z[0], torch.tensor(-1.0)), (x, pt, pt, -1.0), (x, pt, z, None),
                          (torch.zeros(2, 2, 5, 3), torch.zeros(2, 2, 3, 7), torch.zeros(2, 2, 3, 7), -1.0)):
        with pytest.raises(_C.HypadError, match="GPU"):
            f(x_, p_, z_, k=k)
    assert "not" in f.__doc__.lower() and "2 * dist2plane" in f.__doc__ and "math_.py:2125-2159" in f.__doc__
