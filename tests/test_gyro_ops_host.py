"""The rest of the gyrogroup and the metric -- mobius_sub, mobius_coadd, mobius_cosub, geodesic_unit, lambda_x, inner, norm, egrad2rgrad,
sproj, inv_sproj, and antipode, mobius_fn_apply_chain, mobiusify, which need no kernel -- on the host: the restatement of
tests/gyro_ref.py against the reference's own recorded outputs (tests/golden/gyro_ops.npz, written by tests/golden/gen_gyro_ops.py), its
hand-written backward formulas against autograd, the C ABI's declarations, bindings and size checks, and the refusals of the Python
functions -- which come before any device call, so they run here.

The bounds, the two of tests/test_tangent_maps_host.py.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own
fp64 run on every recorded array, relative to max(1, max|array|) (measured worst: 4.2e-7, inner.out); the restatement is held to the fp32
records at the same 1e-6, run in fp64 and in fp32.  The hand formulas are the same arithmetic as autograd's in another order: held to it
at 1e-12 in fp64, on the same scale.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import gyro_ref as gr
from test_tangent_maps_host import _err, _header_signatures

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, HAND_BOUND = 1e-6, 1e-12
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3
# the generator's named rows
ROW_ZERO_X, ROW_ZERO_Y, ROW_RIM_X, ROW_RIM_Y, ROW_SAME, ROW_ZERO_U, ROW_T0, ROW_TNEG, ROW_TBIG = 1, 2, 3, 4, 5, 6, 7, 8, 9
# name: (labels, restatement in the recorded form, hand-written backward, operand keys of the fixture, grad_output key)
CASES = {
    "mobius_sub": (("out", "grad_x", "grad_y"), gr.mobius_sub_ref, gr.mobius_sub_bwd, ("x", "y"), "grad_output"),
    "mobius_coadd": (("out", "grad_x", "grad_y"), gr.mobius_coadd_ref, gr.mobius_coadd_bwd, ("x", "y"), "grad_output"),
    "mobius_cosub": (("out", "grad_x", "grad_y"), gr.mobius_cosub_ref, gr.mobius_cosub_bwd, ("x", "y"), "grad_output"),
    "geodesic_unit": (("out", "grad_t", "grad_x", "grad_u"), gr.geodesic_unit_ref, gr.geodesic_unit_bwd, ("t", "x", "u"), "grad_output"),
    "lambda_x": (("out", "grad_x"), gr.lambda_x_ref, gr.lambda_x_bwd, ("x",), "grad_output"),
    "inner": (("out", "grad_x", "grad_u", "grad_v"), lambda x, u, v: gr.inner_ref(x, u, v, keepdim=True), gr.inner_bwd, ("x", "u", "v"), "grad_output"),
    "norm": (("out", "grad_x", "grad_u"), gr.norm_ref, gr.norm_bwd, ("x", "u"), "grad_output"),
    "egrad2rgrad": (("out", "grad_x", "grad_grad"), gr.egrad2rgrad_ref, gr.egrad2rgrad_bwd, ("x", "v"), "grad_output"),
    "sproj": (("out", "grad_h"), gr.sproj_ref, gr.sproj_bwd, ("h",), "grad_output"),
    "inv_sproj": (("out", "grad_x"), gr.inv_sproj_ref, gr.inv_sproj_bwd, ("x",), "grad_output_wide"),
}
PER_ROW = ("lambda_x", "inner", "norm")                        # one value per row for the result and grad_out
NEW_ENTRY_POINTS = tuple(f"hypad_{n}_{d}" for n in CASES for d in ("fwd", "bwd"))


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "gyro_ops.npz")) as z:
        return {k: z[k] for k in z.files}


def grad_output(go, shape):
    """The fixture's grad_output for a result of `shape`: itself, or its first column for one value per row (the generator's rule)."""
    return go.reshape(shape) if go.numel() == int(np.prod(shape)) else go[:, 0].reshape(shape)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_recorded_reference(dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 for v in fx.values())
    for name, (labels, fn, _, keys, gk) in CASES.items():
        leaves = [torch.from_numpy(fx[k].astype(np.float64)).to(dt).requires_grad_(True) for k in keys]
        o = fn(*leaves)
        assert tuple(o.shape) == fx[f"{name}.out"].shape, (name, tuple(o.shape))
        gs = torch.autograd.grad(o, leaves, grad_output(torch.from_numpy(fx[gk].astype(np.float64)).to(dt), tuple(o.shape)))
        for lab, got in zip(labels, [o.detach()] + list(gs)):
            err = _err(got, fx[f"{name}.{lab}"])
            assert err <= BOUND, (name, lab, str(dt), err)


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    x, y, u, v, t, h = (fx[k].astype(np.float64) for k in ("x", "y", "u", "v", "t", "h"))
    assert x.shape == y.shape == u.shape == v.shape == fx["grad_output"].shape == (10, 5) and t.shape == (10, 1)
    assert h.shape == fx["grad_output_wide"].shape == (10, 6)
    assert len(fx) == 8 + sum(len(c[0]) for c in CASES.values())
    for name, (labels, _, _, keys, _) in CASES.items():
        for lab, k in zip(labels[1:], keys):
            assert fx[f"{name}.{lab}"].shape == fx[k].shape, (name, lab)
    assert fx["inner.out"].shape == (10, 1) and fx["lambda_x.out"].shape == fx["norm.out"].shape == (10,)   # inner: keepdim=True
    assert fx["sproj.out"].shape == (10, 5) and fx["inv_sproj.out"].shape == (10, 6)
    nx, ny, nu, nv = (np.linalg.norm(a, axis=1) for a in (x, y, u, v))
    assert not x[ROW_ZERO_X].any() and not y[ROW_ZERO_Y].any() and not u[ROW_ZERO_U].any() and ROW_ZERO_X != ROW_ZERO_Y
    assert abs(nx[ROW_RIM_X] - 0.9) < 1e-6 and abs(ny[ROW_RIM_Y] - 0.9) < 1e-6 and (x[ROW_SAME] == y[ROW_SAME]).all() and nx[ROW_SAME] > 0
    assert nx.max() <= 0.9 + 1e-6 and ny.max() <= 0.9 + 1e-6 and nu.max() <= 1.5 and 0.1 <= nv.min() and nv.max() <= 1.5
    assert t[ROW_T0, 0] == 0 and t[ROW_TNEG, 0] == -1 and t[ROW_TBIG, 0] == 40 and t.min() == -1 and t.max() == 40
    assert np.delete(t[:, 0], [ROW_T0, ROW_TNEG, ROW_TBIG]).min() >= 0.1 and np.delete(t[:, 0], ROW_TBIG).max() <= 3
    assert abs(np.linalg.norm(fx["geodesic_unit.out"][ROW_TBIG].astype(np.float64)) - 1) <= 1e-6        # the tanh clamp holds at t / 2 = 20
    # h is inv_sproj(y): on the hyperboloid, and sproj brings it back
    assert np.abs((h[:, :5] ** 2).sum(1) - h[:, 5] ** 2 + 1).max() <= 1e-5 * (h[:, 5] ** 2).max()
    assert np.abs(fx["sproj.out"] - y).max() <= 1e-6
    assert all(np.isfinite(a).all() for a in fx.values())


def _hand_data(rows, D, seed, special):
    """x, y, u, v, t (rows, 1), h (rows, D + 1) in fp64.  special, from nine rows on: row 0 with x == y, row 1 zero in both, row 2 a zero x
    alone, row 3 a zero y alone, row 4 a zero tangent u, rows 5 and 6 x and y on the 1 - 1e-3 norm, t = 0, -1 and 40 on rows 6, 7, 8."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda: torch.nn.functional.normalize(torch.randn(rows, D, generator=g, dtype=torch.float64), dim=1)
    x, y, u, v = (unit() * (0.05 + 0.95 * torch.rand(rows, 1, generator=g, dtype=torch.float64)) * s for s in (0.9, 0.9, 1.5, 1.5))
    t = 0.1 + 2.9 * torch.rand(rows, 1, generator=g, dtype=torch.float64)
    if special:
        assert rows >= 9
        y[0] = x[0]
        x[1] = y[1] = 0.0
        x[2] = 0.0
        y[3] = 0.0
        u[4] = 0.0
        x[5] *= (1 - 1e-3) / x[5].norm()
        y[6] *= (1 - 1e-3) / y[6].norm()
        t[6], t[7], t[8] = 0.0, -1.0, 40.0
    return dict(x=x, y=y, u=u, v=v, t=t, h=gr.inv_sproj_ref(y))


def _hand_check(name, ops, tag):
    labels, _, bwd, keys, _ = CASES[name]
    fn = getattr(gr, name + "_ref")
    leaves = [ops[k].clone().requires_grad_(True) for k in keys]
    out = fn(*leaves, keepdim=True) if name in PER_ROW else fn(*leaves)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(len(name)), dtype=torch.float64)
    want = torch.autograd.grad(out, leaves, go)
    with torch.no_grad():
        got = bwd(*(ops[k] for k in keys), go)
    assert len(got) == len(want)
    for lab, a, b in zip(labels[1:], got, want):
        assert a.shape == b.shape and bool(torch.isfinite(a).all()), (name, lab, tag)
        err = _err(a, b)
        assert err <= HAND_BOUND, (name, lab, tag, err)


@pytest.mark.parametrize("rows,D", [(12, 5), (9, 1), (3, 64)])
def test_hand_written_backward_formulas_meet_autograd(rows, D):
    """Ordinary rows, and -- from nine rows on, in a run of their own so that their sizes do not set the scale for the others -- the
    special ones."""
    for special in ((False, True) if rows >= 9 else (False,)):
        ops = _hand_data(rows, D, 100 * rows + D, special)
        for name in CASES:
            _hand_check(name, ops, (rows, D, special))
    # one t shared by every row: its gradient is the sum of the per-row values
    ops = _hand_data(rows, D, 7 * rows + D, False)
    go = torch.randn(rows, D, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for tv in (0.37, -1.0, 40.0, 0.0):
        t = torch.tensor(tv, dtype=torch.float64, requires_grad=True)
        x, u = ops["x"].clone().requires_grad_(True), ops["u"].clone().requires_grad_(True)
        want = torch.autograd.grad(gr.geodesic_unit_ref(t, x, u), [t, x, u], go)
        got = gr.geodesic_unit_bwd(t.detach(), ops["x"], ops["u"], go)
        assert _err(got[0].sum(), want[0]) <= HAND_BOUND and _err(got[1], want[1]) <= HAND_BOUND and _err(got[2], want[2]) <= HAND_BOUND, tv


def test_restated_identities_hold_in_fp64():
    """What tests/test_gpu_gyro_ops.py asks of the library, asked of the yardstick first: every identity to 1e-12 in fp64."""
    from dist_ref import dist_ref
    from tangent_ref import _norm, expmap_ref, mobius_add_ref
    o = _hand_data(33, 5, 5, False)
    x, y, u, v, t = (o[k] * s for k, s in (("x", 0.8 / 0.9), ("y", 0.8 / 0.9), ("u", 1.0), ("v", 1.0), ("t", 1.0)))
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
    assert close(gr.mobius_cosub_ref(mobius_add_ref(x, y), y), x) and close(gr.mobius_coadd_ref(gr.mobius_sub_ref(x, y), y), x)
    assert close(gr.mobius_sub_ref(gr.mobius_coadd_ref(x, y), y), x) and close(mobius_add_ref(gr.mobius_cosub_ref(x, y), y), x)
    assert close(gr.mobius_coadd_ref(x, y), gr.mobius_coadd_ref(y, x)) and close(gr.sproj_ref(gr.inv_sproj_ref(x)), x)
    assert close(gr.inner_ref(x, u, u), gr.norm_ref(x, u) ** 2) and close(gr.inner_ref(x, gr.egrad2rgrad_ref(x, v), u), (v * u).sum(-1))
    assert close(dist_ref(x, gr.geodesic_unit_ref(t, x, u)), t.abs().squeeze(-1))
    assert close(gr.geodesic_unit_ref(t, x, u), expmap_ref(x, t * u / gr.norm_ref(x, u, keepdim=True)))
    assert close(gr.antipode_ref(x), -x) and float(_norm(x).max()) <= 0.8 + 1e-12


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    for cite in ("math_.py:558-589", "math_.py:678-744", "math_.py:747-779", "math_.py:1139-1185", "math_.py:355-383", "math_.py:386-430",
                 "math_.py:433-472", "math_.py:1816-1845", "math_.py:1848-1874", "math_.py:1877-1905"):
        assert cite in text, cite
    header = _header_signatures()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7          # new entry points, no changed one: the version stays
    assert len(NEW_ENTRY_POINTS) == 20 and len(set(NEW_ENTRY_POINTS)) == 20
    for name in NEW_ENTRY_POINTS:
        assert name in header, name
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and args == header[name], (name, args, header[name])
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes == args, name


def test_every_kernel_source_is_built_into_the_library():
    """The new kernels stand in tangent.hip, next to the launch templates they instantiate; whatever source file csrc/ holds is built."""
    from hypad_amd import build
    on_disk = {f for f in os.listdir(build.CSRC) if f.endswith((".hip", ".cpp"))}
    assert on_disk == set(build.DEV_SOURCES) and build.DEV_SOURCES[:len(build.SOURCES)] == build.SOURCES
    text = open(os.path.join(build.CSRC, "tangent.hip")).read()
    assert "tangent.hip" in build.SOURCES and all(f"int {name}(" in text for name in NEW_ENTRY_POINTS)
    assert text.count("void rows2_fwd(") == text.count("void rows2_bwd(") == text.count("int launch2_fwd(") == text.count("int launch2_bwd(") == 1


def test_entry_points_check_their_sizes_before_any_hip_call():
    """Host pointers throughout, on a machine that may have no device: every call below is answered by the argument checks, which come
    before the first HIP call of the entry point (anything later would return a HIP error code instead, or fault on the pointers)."""
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_float * 4096)()
    p, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    plain = [("mobius_sub", 2), ("mobius_coadd", 2), ("mobius_cosub", 2), ("egrad2rgrad", 2), ("lambda_x", 1), ("norm", 2), ("inner", 3)]
    for name, n in plain:
        fwd, bwd = getattr(L, f"hypad_{name}_fwd"), getattr(L, f"hypad_{name}_bwd")
        f = lambda ops=(p,) * (n + 1), rows=4, dim=8: fwd(*ops, n64(rows), dim, None)
        b = lambda ops=(p,) * (n + 1), gr=(p,) * n, rows=4, dim=8: bwd(*ops, *gr, n64(rows), dim, None)
        for call in (f, b):
            assert call(dim=257) == HYPAD_EUNSUPPORTED and call(rows=2 ** 23, dim=256) == HYPAD_EUNSUPPORTED, name
            assert call(rows=-1) == call(dim=0) == call(dim=-3) == HYPAD_EINVAL, name
            for i in range(n + 1):                              # each operand (the last: out or grad_out) missing in turn
                ops = tuple(None if j == i else p for j in range(n + 1))
                assert call(ops=ops) == HYPAD_EINVAL, (name, i)
            assert call(ops=(None,) * (n + 1), rows=0) == 0, name   # no rows: nothing to launch, nothing to read
        assert b(gr=(None,) * n) == 0, name                         # no gradient asked for: nothing to launch
    for name in ("sproj", "inv_sproj"):                             # dim is the ball's width; the limits hold the wider side, dim + 1
        fwd, bwd = getattr(L, f"hypad_{name}_fwd"), getattr(L, f"hypad_{name}_bwd")
        f = lambda ops=(p, p), rows=4, dim=8: fwd(*ops, n64(rows), dim, None)
        b = lambda ops=(p, p), ga=p, rows=4, dim=8: bwd(*ops, ga, n64(rows), dim, None)
        for call in (f, b):
            assert call(dim=256) == call(dim=257) == HYPAD_EUNSUPPORTED and call(rows=2 ** 23, dim=255) == HYPAD_EUNSUPPORTED, name
            assert call(rows=-1) == call(dim=0) == call(dim=-1) == call(dim=-3) == HYPAD_EINVAL, name
            assert call(ops=(None, p)) == call(ops=(p, None)) == HYPAD_EINVAL and call(ops=(None, None), rows=0) == 0, name
        assert b(ga=None) == 0, name
    gf = lambda ops=(p,) * 4, rows=4, dim=8, tc=4: L.hypad_geodesic_unit_fwd(*ops, n64(rows), dim, n64(tc), None)
    gb = lambda ops=(p,) * 4, gr=(p,) * 3, rows=4, dim=8, tc=4: L.hypad_geodesic_unit_bwd(*ops, *gr, n64(rows), dim, n64(tc), None)
    for call in (gf, gb):
        assert call(dim=257) == HYPAD_EUNSUPPORTED and call(rows=2 ** 23, dim=256, tc=1) == HYPAD_EUNSUPPORTED
        assert call(rows=-1) == call(dim=0) == call(tc=3) == call(tc=0) == call(tc=-1) == call(tc=5) == HYPAD_EINVAL
        for i in range(4):
            assert call(ops=tuple(None if j == i else p for j in range(4))) == HYPAD_EINVAL, i
            assert call(ops=tuple(None if j == i else p for j in range(4)), tc=1) == HYPAD_EINVAL, i
        assert call(ops=(None,) * 4, rows=0, tc=1) == HYPAD_EINVAL      # t has its one element even without rows
        assert call(ops=(None,) * 4, rows=0, tc=0) == 0 and call(ops=(p, None, None, None), rows=0, tc=1) == 0
    assert gb(gr=(None,) * 3) == 0


_CALLS = {
    "mobius_sub": lambda g, a, b, **kw: g.mobius_sub(a, b, **kw), "mobius_coadd": lambda g, a, b, **kw: g.mobius_coadd(a, b, **kw),
    "mobius_cosub": lambda g, a, b, **kw: g.mobius_cosub(a, b, **kw), "geodesic_unit": lambda g, a, b, **kw: g.geodesic_unit(0.5, a, b, **kw),
    "inner": lambda g, a, b, **kw: g.inner(a, b, b, **kw), "norm": lambda g, a, b, **kw: g.norm(a, b, **kw),
    "egrad2rgrad": lambda g, a, b, **kw: g.egrad2rgrad(a, b, **kw),
}


def test_python_functions_refuse_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    r, c = torch.zeros(2, 9, 5), torch.zeros(2, 1, 5)
    bad_k = (-0.5, 1.0, 0.0, torch.tensor(-2.0))
    for name, call in _CALLS.items():
        for k in bad_k:
            with pytest.raises(NotImplementedError, match="supported"):
                call(gmath, r, r, k=k)
        for dim in (0, 1, -2):
            with pytest.raises(NotImplementedError, match="supported"):
                call(gmath, r, r, k=-1.0, dim=dim)
        for a, b in ((torch.zeros(4, 257), torch.zeros(4, 257)), (torch.zeros(4, 0), torch.zeros(4, 0)), (r, torch.zeros(2, 9, 4)),
                     (r, torch.zeros(2, 9, 1)), (r, torch.zeros(3, 9, 5)), (r, torch.zeros(2, 8, 5)), (torch.zeros(()), torch.zeros(())),
                     (r.double(), r.double()), (r, r.double()), (torch.zeros(1, 5).expand(2 ** 29, 5), torch.zeros(1, 5))):
            with pytest.raises(NotImplementedError, match="supported"):
                call(gmath, a, b, k=-1.0)
        # what is supported gets as far as the device and is refused there, on host tensors
        for a, b, kw in ((r, r, dict(k=-1.0)), (c, r, dict(k=torch.tensor(-1.0))), (r, c, dict(k=-1.0, dim=2)), (torch.zeros(5), r, dict(k=-1.0)),
                         (torch.zeros(9, 1), torch.zeros(9, 1), dict(k=-1.0, dim=1))):
            with pytest.raises(_C.HypadError, match="GPU"):
                call(gmath, a, b, **kw)
    # the functions of one operand
    for fn, ok, wide, narrow in ((gmath.lambda_x, r, torch.zeros(4, 257), torch.zeros(4, 0)), (gmath.inv_sproj, r, torch.zeros(4, 256), torch.zeros(4, 0)),
                                 (gmath.sproj, torch.zeros(2, 9, 6), torch.zeros(4, 257), torch.zeros(4, 1))):
        for k in bad_k:
            with pytest.raises(NotImplementedError, match="supported"):
                fn(ok, k=k)
        for a, kw in ((ok, dict(dim=0)), (ok, dict(dim=1)), (ok, dict(dim=-2)), (wide, {}), (narrow, {}), (torch.zeros(()), {}), (ok.double(), {}),
                      (torch.zeros(1, 8).expand(2 ** 28, 8), {})):
            with pytest.raises(NotImplementedError, match="supported"):
                fn(a, k=-1.0, **kw)
        for a, kw in ((ok, {}), (ok, dict(dim=2)), (ok[0, 0], {})):
            with pytest.raises(_C.HypadError, match="GPU"):
                fn(a, k=torch.tensor(-1.0), **kw)
    for a in (torch.zeros(4, 255), torch.zeros(4, 1)):              # the widest and the narrowest ball side
        with pytest.raises(_C.HypadError, match="GPU"):
            gmath.inv_sproj(a, k=-1.0)
    for a in (torch.zeros(4, 256), torch.zeros(4, 2)):
        with pytest.raises(_C.HypadError, match="GPU"):
            gmath.sproj(a, k=-1.0)
    # t of geodesic_unit: what geodesic takes
    for t in (torch.zeros(2, 9), torch.zeros(9, 1), torch.zeros(2, 1, 1), torch.zeros(2, 9, 5), torch.zeros(2), torch.zeros(2, 9, 1).double()):
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.geodesic_unit(t, c, r, k=-1.0)
    for t in (0.25, 1, torch.tensor(0.5), torch.zeros(1, 1, 1), torch.zeros(2, 9, 1)):
        with pytest.raises(_C.HypadError, match="GPU"):
            gmath.geodesic_unit(t, c, r, k=-1.0)
    for fn in (gmath.antipode, gmath.mobius_fn_apply_chain, gmath.mobiusify(torch.tanh)):
        with pytest.raises(NotImplementedError):
            fn(r, k=-0.5)
    with pytest.raises(NotImplementedError):
        gmath.mobius_fn_apply_chain(r, torch.tanh, k=-1.0, dim=0)


class _Recorded(torch.autograd.Function):
    """Stands in for _RowScalar on the host: the shape the wrapper gives the result is the wrapper's own."""

    @staticmethod
    def forward(ctx, name, c, *ops):
        return torch.zeros(ops[0].shape[:-1])


def test_results_of_one_value_per_row_have_the_shape_of_the_rows(monkeypatch):
    """inner(keepdim=False) keeps the rows apart: x.shape[:-1] after the broadcast, where the reference returns (rows, rows)."""
    from hypad_amd.hyperspace import gmath
    monkeypatch.setattr(gmath, "_RowScalar", _Recorded)
    x, u = torch.zeros(33, 5), torch.zeros(33, 5)
    assert gmath.inner(x, u, u, k=-1.0).shape == (33,) and gmath.inner(x, u, u, k=-1.0, keepdim=True).shape == (33, 1)
    assert gmath.inner(torch.zeros(2, 1, 5), torch.zeros(2, 9, 5), torch.zeros(5), k=-1.0).shape == (2, 9)
    assert gmath.lambda_x(x, k=-1.0).shape == gmath.norm(x, u, k=-1.0).shape == (33,)
    assert gmath.lambda_x(x, k=-1.0, keepdim=True).shape == gmath.norm(x, u, k=-1.0, keepdim=True).shape == (33, 1)
    assert gr.inner_ref(x, u, u).shape == (33,) and gr.inner_ref(x, u, u, keepdim=True).shape == (33, 1)


def test_functions_without_a_kernel():
    from hypad_amd.hyperspace import gmath
    x = torch.randn(7, 5) * 0.1
    assert torch.equal(gmath.antipode(x, k=-1.0), -x) and torch.equal(gmath.antipode(x, k=torch.tensor(-1.0), dim=-1), -x)
    assert gmath.mobius_fn_apply_chain(x, k=-1.0) is x and gmath.mobius_fn_apply_chain(x) is x       # no function: the identity
    seen = []
    maps = dict(logmap0=lambda a: (seen.append("log"), a + 1.0)[1], expmap0=lambda a: (seen.append("exp"), a * 2.0)[1])
    orig = {n: getattr(gmath, n) for n in maps}
    try:
        for n, f in maps.items():
            setattr(gmath, n, f)
        got = gmath.mobius_fn_apply_chain(x, lambda a: a * 3.0, lambda a: a - 0.5, k=-1.0)
        assert torch.equal(got, ((x + 1.0) * 3.0 - 0.5) * 2.0) and seen == ["log", "exp"]
        fn = gmath.mobiusify(lambda a, s, shift=0.0: a * s + shift)
        assert torch.equal(fn(x, 3.0, k=-1.0, shift=0.25), ((x + 1.0) * 3.0 + 0.25) * 2.0) and seen == ["log", "exp"] * 2
    finally:
        for n, f in orig.items():
            setattr(gmath, n, f)
