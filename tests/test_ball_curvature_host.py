"""PoincareBall(c) at any negative curvature, on the host: the restatement of tests/curvature_ref.py against the reference's own recorded
outputs at k = -0.5 and k = -2 (tests/golden/curvature.npz, written by tests/golden/gen_curvature.py) and, at k = -1, against the
restatements the k = -1 sweeps use; the scaling table the kernels rest on; the C ABI's declarations, bindings and argument checks; and the
refusals of the methods -- which come before any device call, so they run here.

The bounds.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative to
max(1, max|array|); the restatement is held to the fp32 records at the same 1e-6, run in fp64 and in fp32 (the gate of
tests/test_tangent_maps_host.py and tests/test_gyro_ops_host.py).  At k = -1 and under the scaling table the two sides are the same
arithmetic in another order: held at 1e-12 in fp64.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import curvature_ref as cr
from test_tangent_maps_host import _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, SAME_BOUND = 1e-6, 1e-12
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3
# name: (labels, operand set of the fixture, operand keys, grad_output key): the generator's cases
CASES = {
    "project": (("out", "grad_x"), "tan", ("x",), "grad_output"),
    "expmap0": (("out", "grad_u"), "tan", ("u",), "grad_output"),
    "logmap0": (("out", "grad_y"), "nz", ("y",), "grad_output"),
    "mobius_add": (("out", "grad_x", "grad_y"), "tan", ("x", "y"), "grad_output"),
    "mobius_pointwise_mul": (("out", "grad_w", "grad_x"), "tan", ("u", "x"), "grad_output"),
    "mobius_scalar_mul": (("out", "grad_r", "grad_x"), "nz", ("t", "x"), "grad_output"),
    "dist": (("out", "grad_x", "grad_y"), "tan", ("x", "y"), "grad_output"),
    "dist0": (("out", "grad_x"), "tan", ("x",), "grad_output"),
    "expmap": (("out", "grad_x", "grad_u"), "tan", ("x", "u"), "grad_output"),
    "logmap": (("out", "grad_x", "grad_y"), "tan", ("x", "y"), "grad_output"),
    "geodesic": (("out", "grad_t", "grad_x", "grad_y"), "tan", ("t", "x", "y"), "grad_output"),
    "gyration": (("out", "grad_a", "grad_b", "grad_u"), "tan", ("x", "y", "u"), "grad_output"),
    "parallel_transport": (("out", "grad_x", "grad_y", "grad_v"), "tan", ("x", "y", "u"), "grad_output"),
    "parallel_transport0": (("out", "grad_y", "grad_v"), "tan", ("y", "u"), "grad_output"),
    "parallel_transport0back": (("out", "grad_x", "grad_v"), "tan", ("x", "u"), "grad_output"),
    "mobius_sub": (("out", "grad_x", "grad_y"), "gyro", ("x", "y"), "grad_output"),
    "mobius_coadd": (("out", "grad_x", "grad_y"), "gyro", ("x", "y"), "grad_output"),
    "mobius_cosub": (("out", "grad_x", "grad_y"), "gyro", ("x", "y"), "grad_output"),
    "geodesic_unit": (("out", "grad_t", "grad_x", "grad_u"), "gyro", ("t", "x", "u"), "grad_output"),
    "lambda_x": (("out", "grad_x"), "gyro", ("x",), "grad_output"),
    "inner": (("out", "grad_x", "grad_u", "grad_v"), "gyro", ("x", "u", "v"), "grad_output"),
    "norm": (("out", "grad_x", "grad_u"), "gyro", ("x", "u"), "grad_output"),
    "egrad2rgrad": (("out", "grad_x", "grad_grad"), "gyro", ("x", "v"), "grad_output"),
    "sproj": (("out", "grad_h"), "gyro", ("h",), "grad_output"),
    "inv_sproj": (("out", "grad_x"), "gyro", ("x",), "grad_output_wide"),
}
CURVATURES = (0.5, 2.0)
ENTRY_POINTS = tuple(f"hypad_ball_{n}_{d}" for n in CASES for d in ("fwd", "bwd"))
ALIASES = dict(projx="project", transp="parallel_transport", transp0="parallel_transport0", transp0back="parallel_transport0back")


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "curvature.npz")) as z:
        return {k: z[k] for k in z.files}


def grad_output(go, shape):
    """The fixture's grad_output for a result of `shape`: itself, or its first column for one value per row (the generator's rule)."""
    return go.reshape(shape) if go.numel() == int(np.prod(shape)) else go[:, 0].reshape(shape)


def _restated(name, leaves, k):
    fn = cr.FUNCTIONS[name][0]
    return fn(*leaves, k, keepdim=True) if name == "inner" else fn(*leaves, k)


def test_cases_are_the_25_functions():
    assert len(CASES) == 25 and set(CASES) == set(cr.FUNCTIONS) == set(cr.EXPONENTS) and len(ENTRY_POINTS) == 50 == len(set(ENTRY_POINTS))
    for name, (labels, _, keys, _) in CASES.items():
        assert len(labels) == len(keys) + 1 == len(cr.FUNCTIONS[name][1]) + 1 == len(cr.EXPONENTS[name][0]) + 1, name


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("c", CURVATURES)
def test_restatement_meets_the_recorded_reference(c, dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in fx.values())
    for name, (labels, sname, keys, gk) in CASES.items():
        pre = f"c{c:g}."
        leaves = [torch.from_numpy(fx[f"{pre}{sname}.{k}"].astype(np.float64)).to(dt).requires_grad_(True) for k in keys]
        o = _restated(name, leaves, -c)
        assert tuple(o.shape) == fx[f"{pre}{name}.out"].shape, (name, tuple(o.shape))
        gs = torch.autograd.grad(o, leaves, grad_output(torch.from_numpy(fx[f"{pre}{sname}.{gk}"].astype(np.float64)).to(dt), tuple(o.shape)))
        for lab, got in zip(labels, [o.detach()] + list(gs)):
            err = _err(got, fx[f"{pre}{name}.{lab}"])
            assert err <= BOUND, (name, lab, c, str(dt), err)


def test_fixture_holds_the_points_at_the_radius_of_their_ball():
    fx = load_fixture()
    assert len(fx) == 2 * (5 + 8 + 5 + sum(len(c[0]) for c in CASES.values()))
    for c in CURVATURES:
        tan = {k: fx[f"c{c:g}.tan.{k}"].astype(np.float64) for k in ("x", "y", "u", "t")}
        gyro = {k: fx[f"c{c:g}.gyro.{k}"].astype(np.float64) for k in ("x", "y", "u", "v", "t", "h")}
        nz = {k: fx[f"c{c:g}.nz.{k}"].astype(np.float64) for k in ("x", "y", "t")}
        rim = 0.9 / math.sqrt(c)
        for ops in (tan, gyro):
            nx, ny = np.linalg.norm(ops["x"], axis=1), np.linalg.norm(ops["y"], axis=1)
            assert ops["x"].shape == (10, 5) and abs(nx.max() - rim) < 1e-6 and abs(ny.max() - rim) < 1e-6
        assert np.linalg.norm(tan["x"] - tan["y"], axis=1).min() >= 0.1 / math.sqrt(c)        # dist and logmap see no x == y row
        assert (gyro["x"][5] == gyro["y"][5]).all() and gyro["t"].max() == 40 and not gyro["u"][6].any()
        assert nz["x"].shape == (8, 5) and np.linalg.norm(nz["x"], axis=1).min() > 0 and np.linalg.norm(nz["y"], axis=1).min() > 0
        assert np.linalg.norm(tan["x"], axis=1).min() == 0 and np.linalg.norm(tan["y"], axis=1).min() == 0
        h = gyro["h"]                                                # on the hyperboloid of curvature -c: |h_space|^2 - h_time^2 = -1 / c
        assert gyro["h"].shape == (10, 6) and np.abs((h[:, :5] ** 2).sum(1) - h[:, 5] ** 2 + 1 / c).max() <= 1e-5 * (h[:, 5] ** 2).max()
        assert np.abs(fx[f"c{c:g}.sproj.out"] - gyro["y"]).max() <= 1e-6


def _k1_data():
    out = {}
    for f in ("tangent_maps", "gyro_ops"):
        with np.load(os.path.join(ROOT, "tests", "golden", f + ".npz")) as z:
            out[f] = {k: torch.from_numpy(z[k].astype(np.float64)) for k in ("x", "y", "u", "t")}
    with np.load(os.path.join(ROOT, "tests", "golden", "gyro_ops.npz")) as z:
        out["gyro_ops"].update(v=torch.from_numpy(z["v"].astype(np.float64)), h=torch.from_numpy(z["h"].astype(np.float64)))
    return out


def test_at_k_minus_one_it_is_the_restatements_of_the_k_minus_one_sweeps():
    import dist_ref
    import gyro_ref as gr
    import tangent_ref as tr
    data = _k1_data()
    for ops in data.values():
        x, y, u, t = ops["x"], ops["y"], ops["u"], ops["t"]
        pairs = [(cr.expmap(x, u, -1.0), tr.expmap_ref(x, u)), (cr.logmap(x, y, -1.0), tr.logmap_ref(x, y)),
                 (cr.geodesic(t, x, y, -1.0), tr.geodesic_ref(t, x, y)), (cr.gyration(x, y, u, -1.0), tr.gyration_ref(x, y, u)),
                 (cr.parallel_transport(x, y, u, -1.0), tr.parallel_transport_ref(x, y, u)),
                 (cr.parallel_transport0(y, u, -1.0), tr.parallel_transport0_ref(y, u)),
                 (cr.parallel_transport0back(x, u, -1.0), tr.parallel_transport0back_ref(x, u)),
                 (cr.mobius_add(x, y, -1.0), tr.mobius_add_ref(x, y)), (cr.mobius_scalar_mul(t, x, -1.0), tr.mobius_scalar_mul_ref(t, x)),
                 (cr.mobius_sub(x, y, -1.0), gr.mobius_sub_ref(x, y)), (cr.mobius_coadd(x, y, -1.0), gr.mobius_coadd_ref(x, y)),
                 (cr.mobius_cosub(x, y, -1.0), gr.mobius_cosub_ref(x, y)), (cr.geodesic_unit(t, x, u, -1.0), gr.geodesic_unit_ref(t, x, u)),
                 (cr.lambda_x(x, -1.0), gr.lambda_x_ref(x)), (cr.inner(x, u, y, -1.0), gr.inner_ref(x, u, y)),
                 (cr.norm(x, u, -1.0, keepdim=True), gr.norm_ref(x, u, keepdim=True)), (cr.egrad2rgrad(x, u, -1.0), gr.egrad2rgrad_ref(x, u)),
                 (cr.inv_sproj(x, -1.0), gr.inv_sproj_ref(x)), (cr.sproj(gr.inv_sproj_ref(y), -1.0), gr.sproj_ref(gr.inv_sproj_ref(y))),
                 (cr.dist(x, y, -1.0), dist_ref.dist_ref(x, y)), (cr.dist0(x, -1.0, keepdim=True), dist_ref.dist0_ref(x, keepdim=True))]
        for i, (got, want) in enumerate(pairs):
            assert got.shape == want.shape and _err(got, want) <= SAME_BOUND, (i, _err(got, want))
        # project, expmap0, logmap0, mobius_pointwise_mul: the formulas of oracle/gmath.py's k = -1 functions, stated here
        n = u.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        assert _err(cr.expmap0(u, -1.0), torch.tanh(n.clamp_max(15)) * u / n) <= SAME_BOUND
        ny = y.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        assert _err(cr.logmap0(y, -1.0), torch.atanh(ny.clamp_max(1 - 1e-7)) * y / ny) <= SAME_BOUND
        far = 1.5 * x / x.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        assert torch.equal(cr.project(x, -1.0), x) and _err(cr.project(far, -1.0).norm(dim=-1), (1 - 4e-3) * (far.norm(dim=-1) > 0).double()) <= SAME_BOUND
        assert _err(cr.antipode(x, -1.0), -x) == 0


@pytest.mark.parametrize("c", [0.25, 0.5, 2.0, 7.3, 100.0])
def test_scaling_table_carries_curvature_c_onto_curvature_one(c):
    """f_c(a_0, ...) = s^eo f_1(s^e0 a_0, ...), s = sqrt(c): the identity the kernels rest on, in fp64 on outputs and on every operand
    gradient, with points out to 0.999 / sqrt(c) (no all-zero and no coincident rows: there artanh(n) / n is decided by rounding)."""
    g = torch.Generator().manual_seed(int(c * 100))
    s, rows, D = math.sqrt(c), 12, 5
    unit = lambda: torch.nn.functional.normalize(torch.randn(rows, D, generator=g, dtype=torch.float64), dim=1)
    radius = torch.rand(rows, 1, generator=g, dtype=torch.float64) * 0.9 + 0.05
    radius[0] = 0.999
    ops = dict(x=unit() * radius / s, y=unit() * radius.flip(0) / s, a=unit() * radius / s, b=unit() * radius.flip(0) / s,
               u=unit() * 1.3, v=unit() * 0.7, grad=unit(), w=torch.randn(rows, D, generator=g, dtype=torch.float64),
               t=torch.rand(rows, 1, generator=g, dtype=torch.float64) * 2 - 0.5, r=torch.rand(rows, 1, generator=g, dtype=torch.float64) * 3 - 1)
    ops["h"] = cr.inv_sproj(ops["y"], -c)
    for name, (fn, keys, _) in cr.FUNCTIONS.items():
        exps, eo = cr.EXPONENTS[name]
        kw = dict(keepdim=True) if name in ("inner", "norm", "lambda_x", "dist", "dist0") else {}
        la = [ops[k].clone().requires_grad_(True) for k in keys]
        lb = [ops[k].clone().requires_grad_(True) for k in keys]
        oa = fn(*la, -c, **kw)
        ob = s ** eo * fn(*(s ** e * t for e, t in zip(exps, lb)), -1.0, **kw)
        go = torch.randn(oa.shape, generator=g, dtype=torch.float64)
        ga, gb = torch.autograd.grad(oa, la, go), torch.autograd.grad(ob, lb, go)
        for lab, p, q in zip(("out",) + keys, (oa.detach(),) + ga, (ob.detach(),) + gb):
            assert _err(p, q) <= 1e-9, (name, lab, c, _err(p, q))


def _signatures():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    sigs = {}
    for m in re.finditer(r"\bint (hypad_\w+)\(([^)]*)\)\s*;", text):
        kinds = []
        for a in m.group(2).split(","):
            a = a.strip()
            kinds.append(ctypes.c_void_p if "*" in a or a.startswith("hypad_stream_t") else ctypes.c_int64 if a.startswith("int64_t") else
                         ctypes.c_int if a.startswith("int ") else ctypes.c_double if a.startswith("double ") else None)
        sigs[m.group(1)] = kinds
    return sigs


def test_header_declares_and_the_binding_binds_the_50_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert "docs/history/curvature.md" in text and "f_c(a_0, a_1, ...) = s^eo f_1(s^e0 a_0, s^e1 a_1, ...)" in text
    header = _signatures()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7          # new entry points, no changed one: the version stays
    source = open(os.path.join(ROOT, "hypad_amd", "csrc", "tangent.hip")).read()
    for name in ENTRY_POINTS:
        assert name in header and f"int {name}(" in source, name
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and args == header[name] and None not in args, (name, args, header[name])
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes == args, name
        k1 = header[name.replace("hypad_ball_", "hypad_")]                # the k = -1 argument list plus `double c` before the stream
        if name.split("_ball_")[1].rsplit("_", 1)[0] in ("mobius_add", "mobius_pointwise_mul"):
            k1 = k1[:-2] + k1[-1:]                                        # (their one-row broadcast count is not taken)
        assert args == k1[:-1] + [ctypes.c_double, ctypes.c_void_p], name
    # one copy of each kernel template, shared by the curved and the k = -1 instantiations
    for t in ("rows1", "rows2", "rows3", "rowst", "rowsr", "rows_scalar", "proj"):
        assert source.count(f"void {t}_fwd(") == source.count(f"void {t}_bwd(") == 1, t


def test_entry_points_check_c_and_their_sizes_before_any_hip_call():
    """Host pointers throughout, on a machine that may have no device: every call below is answered by the argument checks."""
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_float * 4096)()
    p, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    nops = {n: len(c[2]) for n, c in CASES.items()}
    timed = {"geodesic": 3, "geodesic_unit": 3, "mobius_scalar_mul": 2}
    for name, n in nops.items():
        fwd, bwd = getattr(L, f"hypad_ball_{name}_fwd"), getattr(L, f"hypad_ball_{name}_bwd")
        tail = (lambda rows: (n64(rows),)) if name in timed else (lambda rows: ())
        f = lambda rows=4, dim=8, c=0.5, ops=None: fwd(*(ops or (p,) * (n + 1)), n64(rows), dim, *tail(rows), ctypes.c_double(c), None)
        b = lambda rows=4, dim=8, c=0.5, ops=None, gr=None: bwd(*(ops or (p,) * (n + 1)), *(gr or (p,) * n), n64(rows), dim, *tail(rows),
                                                                ctypes.c_double(c), None)
        for call in (f, b):
            for c in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
                assert call(c=c) == HYPAD_EINVAL, (name, c)
            assert call(c=float("nan"), dim=257) == HYPAD_EINVAL, name             # c first
            assert call(dim=257) == HYPAD_EUNSUPPORTED and call(rows=2 ** 23, dim=256) == HYPAD_EUNSUPPORTED, name
            assert call(rows=-1) == call(dim=0) == call(dim=-3) == HYPAD_EINVAL, name
            for i in range(n + 1):                              # each operand (the last: out or grad_out) missing in turn
                assert call(ops=tuple(None if j == i else p for j in range(n + 1))) == HYPAD_EINVAL, (name, i)
            if name not in timed:
                assert call(ops=(None,) * (n + 1), rows=0) == 0, name   # no rows: nothing to launch, nothing to read
        assert b(gr=(None,) * n) == 0, name                             # no gradient asked for: nothing to launch
        if name in ("sproj", "inv_sproj"):                              # dim is the ball's width; the limits hold the wider side
            assert f(dim=256) == b(dim=256) == HYPAD_EUNSUPPORTED and f(dim=255, rows=0) == 0, name
    for name in timed:                                                   # the count of t / r: 1, or one per row
        fwd = getattr(L, f"hypad_ball_{name}_fwd")
        call = lambda tc, rows=4: fwd(*(p,) * (timed[name] + 1), n64(rows), 8, n64(tc), ctypes.c_double(2.0), None)
        assert call(3) == call(0) == call(-1) == call(5) == HYPAD_EINVAL, name


_R, _C1 = torch.zeros(2, 9, 5), torch.zeros(2, 1, 5)
# method: (a supported call's operands, then keyword arguments)
_SUPPORTED = {
    "project": ((_R,), {}), "expmap0": ((_R,), {}), "logmap0": ((_R,), {}), "dist0": ((_R,), {}), "lambda_x": ((_R,), {}),
    "sproj": ((torch.zeros(2, 9, 6),), {}), "inv_sproj": ((_R,), {}), "mobius_add": ((_R, _C1), {}), "mobius_sub": ((_R, _C1), {}),
    "mobius_coadd": ((_C1, _R), {}), "mobius_cosub": ((_R, _R), {}), "dist": ((_R, _R), {}), "expmap": ((_R, torch.zeros(5)), {}),
    "logmap": ((_C1, _R), {}), "parallel_transport0": ((_R, _R), {}), "parallel_transport0back": ((_R, _R), {}), "norm": ((_R, _R), dict(keepdim=True)),
    "egrad2rgrad": ((_R, _R), {}), "mobius_scalar_mul": ((0.5, _R), {}), "mobius_pointwise_mul": ((torch.zeros(5), _R), {}),
    "geodesic": ((0.25, _R, _C1), {}), "geodesic_unit": ((torch.zeros(2, 9, 1), _R, _R), {}), "gyration": ((_R, _R, _C1), {}),
    "parallel_transport": ((_R, _C1, _R), {}), "inner": ((_R, _R, _R), {}),
}


def test_every_method_refuses_a_bad_c_before_anything_else():
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    assert set(_SUPPORTED) == set(CASES)
    for c in (0.0, -1.0, float("inf"), float("nan")):
        ball = PoincareBall(c)
        for name, (ops, kw) in _SUPPORTED.items():
            with pytest.raises(NotImplementedError, match="c = "):
                getattr(ball, name)(*ops, **kw)
        with pytest.raises(NotImplementedError, match="c = "):
            ball.antipode(_R)
    ball = PoincareBall(0.5)
    ball.c = torch.tensor(0.5, requires_grad=True)                       # learnable curvature is not part of this
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(NotImplementedError, match="requires grad"):
            getattr(ball, name)(*ops, **kw)
    ball.c = torch.tensor([0.5, 2.0])
    with pytest.raises(NotImplementedError, match="one value"):
        ball.expmap(_R, _R)


@pytest.mark.parametrize("c", [0.5, 1.0, 7.3])
def test_supported_calls_get_as_far_as_the_device_and_bad_operands_do_not(c):
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    ball = PoincareBall(c)
    # the constructor stays as it is
    assert ball.c.device.type == "cpu" and ball.c.dtype == torch.float32 and float(ball.c) == float(torch.tensor(c)) == -float(ball.k)
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(_C.HypadError, match="GPU"):
            getattr(ball, name)(*ops, **kw)
        with pytest.raises(_C.HypadError, match="GPU"):
            getattr(ball, name)(*ops, dim=2, **kw)
        for dim in (0, 1, -2):                                            # the last dimension only
            with pytest.raises(NotImplementedError, match="supported"):
                getattr(ball, name)(*ops, dim=dim, **kw)
        wide = tuple(torch.zeros(4, 257) if isinstance(t, torch.Tensor) and t.shape[-1] in (5, 6) else
                     torch.zeros(4, 1) if isinstance(t, torch.Tensor) else t for t in ops)
        with pytest.raises(NotImplementedError, match="supported"):       # D <= 256
            getattr(ball, name)(*wide, **kw)
    strict = [n for n in _SUPPORTED if n not in ("project", "expmap0", "logmap0", "mobius_add", "mobius_pointwise_mul", "mobius_scalar_mul")]
    for name in strict:                                                   # fp32 where gmath demands it
        ops, kw = _SUPPORTED[name]
        with pytest.raises(NotImplementedError, match="supported"):
            getattr(ball, name)(*(t.double() if isinstance(t, torch.Tensor) else t for t in ops), **kw)
    for name in ("project", "expmap0", "logmap0"):                        # ... and a cast where gmath casts
        with pytest.raises(_C.HypadError, match="GPU"):
            getattr(ball, name)(_R.double())
    with pytest.raises(_C.HypadError, match="GPU"):
        ball.mobius_add(_R.double(), _C1.half())
    # the projections' ball side: 1 to 255
    for fn, ok, bad in ((ball.inv_sproj, torch.zeros(4, 255), torch.zeros(4, 256)), (ball.sproj, torch.zeros(4, 256), torch.zeros(4, 1))):
        with pytest.raises(_C.HypadError, match="GPU"):
            fn(ok)
        with pytest.raises(NotImplementedError, match="supported"):
            fn(bad)
    # operands that do not fit each other
    for name in ("mobius_sub", "expmap", "logmap", "norm", "egrad2rgrad", "parallel_transport0"):
        for a, b in ((_R, torch.zeros(2, 9, 4)), (_R, torch.zeros(3, 9, 5)), (torch.zeros(()), torch.zeros(()))):
            with pytest.raises(NotImplementedError, match="supported"):
                getattr(ball, name)(a, b)
    with pytest.raises(NotImplementedError, match="supported"):
        ball.dist(_R, _C1)                                                # dist broadcasts nothing
    with pytest.raises(NotImplementedError):
        ball.mobius_pointwise_mul(torch.zeros(9, 5), _R)
    for t in (torch.zeros(2, 9), torch.zeros(9, 1), torch.zeros(2, 9, 5)):
        with pytest.raises(NotImplementedError, match="supported"):
            ball.geodesic(t, _R, _R)
        with pytest.raises(NotImplementedError, match="supported"):
            ball.mobius_scalar_mul(t, _R)
    with pytest.raises(NotImplementedError, match="eps"):
        ball.project(_R, eps=1e-3)
    # batches of no rows get as far as the device too
    with pytest.raises(_C.HypadError, match="GPU"):
        ball.expmap(torch.zeros(0, 5), torch.zeros(0, 5))


def test_at_c_one_a_method_is_the_gmath_function(monkeypatch):
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    ball, seen = PoincareBall(1.0), []
    for name in _SUPPORTED:
        monkeypatch.setattr(gmath, name, lambda *a, _n=name, **kw: seen.append((_n, kw.get("k"))) or _n)
    for name, (ops, kw) in _SUPPORTED.items():
        assert getattr(ball, name)(*ops, **kw) == name
    assert seen == [(n, -1.0) for n in _SUPPORTED]
    seen.clear()
    other = PoincareBall(0.5)
    with pytest.raises(Exception, match="GPU"):
        other.expmap(_R, _R)
    assert seen == []                                                     # any other c does not go through gmath's function


def test_antipode_and_the_aliases():
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    x = torch.randn(7, 5) * 0.1
    for c in (0.5, 1.0, 2.0):
        assert torch.equal(PoincareBall(c).antipode(x), -x) and torch.equal(PoincareBall(c).antipode(x, dim=-1), -x)
    for alias, name in ALIASES.items():
        assert getattr(PoincareBall, alias) is getattr(PoincareBall, name), alias
    assert all(callable(getattr(PoincareBall, n)) for n in list(CASES) + ["antipode"])
    assert "project" in PoincareBall.__doc__ and "implicitly" in PoincareBall.__doc__
