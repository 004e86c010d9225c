"""The tangent maps expmap, logmap, geodesic, gyration, parallel_transport, parallel_transport0 and parallel_transport0back on the host:
the restatement of tests/tangent_ref.py against the reference's own recorded outputs (tests/golden/tangent_maps.npz, written by
tests/golden/gen_tangent_maps.py), its hand-written backward formulas against autograd, the C ABI's declarations, bindings and size
checks, and the refusals of the Python functions -- which come before any device call, so they run here.

The bounds.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative
to max(1, max|array|) (measured worst: 1.9e-7, logmap.out); the restatement is held to the fp32 records at the same 1e-6, run in fp64
and in fp32.  The hand formulas are the same arithmetic as autograd's in another order: held to it at 1e-12 in fp64, on the same scale.
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import tangent_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, HAND_BOUND = 1e-6, 1e-12
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3
# the generator's named rows
ROW_ZERO_X, ROW_ZERO_Y, ROW_RIM_X, ROW_RIM_Y, ROW_ZERO_U, ROW_LONG_U, ROW_T0, ROW_T1, ROW_TNEG = 1, 2, 3, 4, 5, 6, 7, 8, 9
# name: (labels, restatement, hand-written backward, operand keys of the fixture)
CASES = {
    "expmap": (("out", "grad_x", "grad_u"), tr.expmap_ref, tr.expmap_bwd, ("x", "u")),
    "logmap": (("out", "grad_x", "grad_y"), tr.logmap_ref, tr.logmap_bwd, ("x", "y")),
    "geodesic": (("out", "grad_t", "grad_x", "grad_y"), tr.geodesic_ref, tr.geodesic_bwd, ("t", "x", "y")),
    "gyration": (("out", "grad_a", "grad_b", "grad_u"), tr.gyration_ref, tr.gyration_bwd, ("x", "y", "u")),
    "parallel_transport": (("out", "grad_x", "grad_y", "grad_v"), tr.parallel_transport_ref, tr.parallel_transport_bwd, ("x", "y", "u")),
    "parallel_transport0": (("out", "grad_y", "grad_v"), tr.parallel_transport0_ref, tr.parallel_transport0_bwd, ("y", "u")),
    "parallel_transport0back": (("out", "grad_x", "grad_v"), tr.parallel_transport0back_ref, tr.parallel_transport0back_bwd, ("x", "u")),
}
NEW_ENTRY_POINTS = tuple(f"hypad_{n}_{d}" for n in CASES for d in ("fwd", "bwd"))


def load_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "tangent_maps.npz")) as z:
        return {k: z[k] for k in z.files}


def _err(got, want):
    want = want.double().numpy() if isinstance(want, torch.Tensor) else np.asarray(want, dtype=np.float64)
    return float(np.abs(got.double().numpy() - want).max()) / max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
def test_restatement_meets_the_recorded_reference(dt):
    fx = load_fixture()
    assert all(v.dtype == np.float32 for v in fx.values())
    for name, (labels, fn, _, keys) in CASES.items():
        leaves = [torch.from_numpy(fx[k].astype(np.float64)).to(dt).requires_grad_(True) for k in keys]
        o = fn(*leaves)
        assert tuple(o.shape) == fx[f"{name}.out"].shape, (name, tuple(o.shape))
        gs = torch.autograd.grad(o, leaves, torch.from_numpy(fx["grad_output"].astype(np.float64)).to(dt))
        for lab, got in zip(labels, [o.detach()] + list(gs)):
            err = _err(got, fx[f"{name}.{lab}"])
            assert err <= BOUND, (name, lab, str(dt), err)


def test_fixture_holds_the_cases_the_tests_name():
    fx = load_fixture()
    x, y, u, t = (fx[k].astype(np.float64) for k in ("x", "y", "u", "t"))
    assert x.shape == y.shape == u.shape == fx["grad_output"].shape == (10, 5) and t.shape == (10, 1)
    assert len(fx) == 5 + sum(len(c[0]) for c in CASES.values())
    for name, (labels, _, _, keys) in CASES.items():
        for lab, k in zip(labels, ("x",) + keys):                  # (out has the shape of a row operand)
            assert fx[f"{name}.{lab}"].shape == fx[k].shape, (name, lab)
    nx, ny, nu = (np.linalg.norm(a, axis=1) for a in (x, y, u))
    assert not x[ROW_ZERO_X].any() and not y[ROW_ZERO_Y].any() and not u[ROW_ZERO_U].any() and ROW_ZERO_X != ROW_ZERO_Y
    assert abs(nx[ROW_RIM_X] - 0.9) < 1e-6 and abs(ny[ROW_RIM_Y] - 0.9) < 1e-6 and abs(nu[ROW_LONG_U] - 12) < 1e-5
    assert nx.max() <= 0.9 + 1e-6 and ny.max() <= 0.9 + 1e-6 and np.delete(nu, ROW_LONG_U).max() <= 1.5
    assert 12 / (1 - nx[ROW_LONG_U] ** 2) > 15 and abs(np.linalg.norm(fx["expmap.out"][ROW_LONG_U].astype(np.float64)) - 1) <= 1e-6
    assert t[ROW_T0, 0] == 0 and t[ROW_T1, 0] == 1 and t[ROW_TNEG, 0] == -0.25 and t.min() == -0.25 and t.max() == 1
    assert float(np.linalg.norm(x - y, axis=1).min()) >= 0.1       # no x == y row: see the generator
    assert all(np.isfinite(v).all() for v in fx.values())


def _hand_data(rows, D, seed):
    """x, y, u, t (rows, 1), grad_out in fp64: from eight rows on, rows 0 and 1 with x == y at norms 0.3 and 0.6, row 2 zero in both, row 3
    a zero x alone, row 4 a zero tangent, row 5 a tangent of norm 12 at |x| = 0.6, t = 0, 1, -0.25 on rows 5, 6, 7."""
    g = torch.Generator().manual_seed(seed)
    unit = lambda: torch.nn.functional.normalize(torch.randn(rows, D, generator=g, dtype=torch.float64), dim=1)
    x, y, u = (unit() * torch.rand(rows, 1, generator=g, dtype=torch.float64) * s for s in (0.9, 0.9, 1.5))
    t = 0.1 + 0.8 * torch.rand(rows, 1, generator=g, dtype=torch.float64)
    if rows >= 8:
        x[0] *= 0.3 / x[0].norm()
        x[1] *= 0.6 / x[1].norm()
        y[0], y[1] = x[0], x[1]
        x[2] = y[2] = 0.0
        x[3] = 0.0
        u[4] = 0.0
        x[5] *= 0.6 / x[5].norm()
        u[5] *= 12 / u[5].norm()
        t[5], t[6], t[7] = 0.0, 1.0, -0.25
    return dict(x=x, y=y, u=u, t=t), torch.randn(rows, D, generator=g, dtype=torch.float64)


@pytest.mark.parametrize("rows,D", [(12, 5), (9, 1), (3, 64)])
def test_hand_written_backward_formulas_meet_autograd(rows, D):
    ops, go = _hand_data(rows, D, 100 * rows + D)
    for name, (labels, fn, bwd, keys) in CASES.items():
        leaves = [ops[k].clone().requires_grad_(True) for k in keys]
        want = torch.autograd.grad(fn(*leaves), leaves, go)
        with torch.no_grad():
            got = bwd(*(ops[k] for k in keys), go)
        assert len(got) == len(want)
        for lab, a, b in zip(labels[1:], got, want):
            assert a.shape == b.shape and bool(torch.isfinite(a).all()), (name, lab)
            err = _err(a, b)
            assert err <= HAND_BOUND, (name, lab, err)
    # one t shared by every row: its gradient is the sum of the per-row values
    t = torch.tensor(0.37, dtype=torch.float64, requires_grad=True)
    x, y = ops["x"].clone().requires_grad_(True), ops["y"].clone().requires_grad_(True)
    want = torch.autograd.grad(tr.geodesic_ref(t, x, y), [t, x, y], go)
    got = tr.geodesic_bwd(t.detach(), ops["x"], ops["y"], go)
    assert _err(got[0].sum(), want[0]) <= HAND_BOUND and _err(got[1], want[1]) <= HAND_BOUND and _err(got[2], want[2]) <= HAND_BOUND


def test_log1p_form_follows_the_limit_where_the_logarithm_pair_returns_zero():
    """The one deliberate difference from the reference, on a near-coincident pair in fp32: x = 0 and |y| = 1.7e-8, below half the
    spacing of fp32 under 1, so log(1 + n) - log(1 - n) is exactly 0 -- the reference's logmap returns the zero vector, its geodesic
    stays at x -- while the log1p form returns what the fp64 run gives: logmap(0, y) = y, geodesic(t, 0, y) = t y."""
    x = torch.zeros(1, 3)
    y = torch.tensor([[1e-8, -1e-8, 1e-8]])
    n = tr._norm(tr.mobius_add_ref(-x, y))
    assert float(n) > 0 and float(torch.log(1 + n) - torch.log(1 - n)) == 0.0
    assert float((tr.logmap_ref(x, y) - y).abs().max()) <= 1e-6 * float(n)
    assert float((tr.logmap_ref(x, y).double() - tr.logmap_ref(x.double(), y.double())).abs().max()) <= 1e-6 * float(n)
    t = torch.tensor([[0.25]])
    assert float((tr.geodesic_ref(t, x, y) - 0.25 * y).abs().max()) <= 1e-6 * float(n)


def _header_signatures():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    sigs = {}
    for m in re.finditer(r"\bint (hypad_\w+)\(([^)]*)\)\s*;", text):
        args = []
        for a in m.group(2).split(","):
            a = a.strip()
            args.append(ctypes.c_void_p if "*" in a or a.startswith("hypad_stream_t") else ctypes.c_int64 if a.startswith("int64_t") else
                        ctypes.c_int if a.startswith("int ") else None)
        sigs[m.group(1)] = args
    return sigs


def test_header_declares_and_the_binding_binds_the_new_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert re.search(r"#define HYPAD_ABI_VERSION 7\b", text)
    for cite in ("math_.py:1052-1102", "math_.py:1188-1230", "math_.py:978-1049", "math_.py:592-675", "math_.py:1669-1746", "math_.py:1749-1779",
                 "math_.py:1782-1813"):
        assert cite in text, cite
    header = _header_signatures()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7
    assert len(NEW_ENTRY_POINTS) == 14
    for name in NEW_ENTRY_POINTS:
        assert name in header, name
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and args == header[name], (name, args, header[name])
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes == args, name


def test_tangent_source_is_built_into_the_library():
    from hypad_amd import build
    assert "tangent.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "tangent.hip"))


def test_entry_points_check_their_sizes_before_any_hip_call():
    """Host pointers throughout, on a machine that may have no device: every call below is answered by the argument checks, which come
    before the first HIP call of the entry point (anything later would return a HIP error code instead, or fault on the pointers)."""
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_float * 4096)()
    p, n64 = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64
    two = [("expmap", 2), ("logmap", 2), ("parallel_transport0", 2), ("parallel_transport0back", 2), ("gyration", 3), ("parallel_transport", 3)]
    for name, n in two:
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
    gf = lambda ops=(p,) * 4, rows=4, dim=8, tc=4: L.hypad_geodesic_fwd(*ops, n64(rows), dim, n64(tc), None)
    gb = lambda ops=(p,) * 4, gr=(p,) * 3, rows=4, dim=8, tc=4: L.hypad_geodesic_bwd(*ops, *gr, n64(rows), dim, n64(tc), None)
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
    "expmap": lambda g, a, b, **kw: g.expmap(a, b, **kw), "logmap": lambda g, a, b, **kw: g.logmap(a, b, **kw),
    "geodesic": lambda g, a, b, **kw: g.geodesic(0.5, a, b, **kw), "gyration": lambda g, a, b, **kw: g.gyration(a, b, b, **kw),
    "parallel_transport": lambda g, a, b, **kw: g.parallel_transport(a, b, b, **kw),
    "parallel_transport0": lambda g, a, b, **kw: g.parallel_transport0(a, b, **kw),
    "parallel_transport0back": lambda g, a, b, **kw: g.parallel_transport0back(a, b, **kw),
}


def test_python_functions_refuse_before_any_device_call():
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    assert set(_CALLS) == set(CASES)
    r, c = torch.zeros(2, 9, 5), torch.zeros(2, 1, 5)
    for name, call in _CALLS.items():
        for k in (-0.5, 1.0, 0.0, torch.tensor(-2.0)):
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
    for t in (torch.zeros(2, 9), torch.zeros(9, 1), torch.zeros(2, 1, 1), torch.zeros(2, 9, 5), torch.zeros(2), torch.zeros(2, 9, 1).double()):
        with pytest.raises(NotImplementedError, match="supported"):
            gmath.geodesic(t, c, r, k=-1.0)
    for t in (0.25, 1, torch.tensor(0.5), torch.zeros(1, 1, 1), torch.zeros(2, 9, 1)):
        with pytest.raises(_C.HypadError, match="GPU"):
            gmath.geodesic(t, c, r, k=-1.0)
    # the new names stand next to the maps at the origin, which keep theirs
    for name in ("expmap0", "logmap0", "mobius_add", "dist", "mobius_scalar_mul", "weighted_midpoint"):
        assert callable(getattr(gmath, name))
    with pytest.raises(TypeError):
        gmath.expmap0(r, r, k=-1.0)
