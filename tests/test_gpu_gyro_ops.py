"""mobius_sub, mobius_coadd, mobius_cosub, geodesic_unit, lambda_x, inner, norm, egrad2rgrad, sproj and inv_sproj on the GPU
(hypad_<name>_fwd / _bwd of csrc/tangent.hip; hyperspace/gmath runs them) against the plain-torch restatement of tests/gyro_ref.py --
which tests/test_gyro_ops_host.py pins to the reference's own outputs -- run in fp64 and fp32 on the CPU, under the project's rule
``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1).  No tolerance of its own.

The data (``_data``).  Points x and y within radius 0.9, tangents u and v with norms in [0.1, 1.5], t (rows, 1) in [0.1, 3], h =
inv_sproj(y) computed in fp64, grad_out ~ N(0, 1) in the shape of each result.  The special rows get tests of their own and do not set
err32 for the others: x == y, both operands zero, points on the 1 - 1e-3 norm, a zero tangent, t = 0, -1 and 40.

The kernels have no tile: a wave per row, 64 lanes x 4 elements, four waves a workgroup, at most 4 096 workgroups a launch.  So the
shapes are rows 1, 4 and 5 (a workgroup's waves not filled, filled, one past), 16 385 = 4 * 4 096 + 1 (one row past a single grid pass)
and D = 1, 63, 64, 65, 255, 256 (one to four elements a lane, the last lane empty or full); for the projections, whose two sides differ
by one column, ball widths 1, 63, 64 and 255 (the extra column lands in a new lane element at 64 -> 65 and fills the last one at 256).

The identities compare two results of the library with each other; each side is off its own fp64 value by at most the rule's
allowance for it (C * err32 + F with the restatement's err32 for that side), so the two may differ by the sum of the two allowances.
"""
import pytest
import torch

import gyro_ref as gr
import tangent_ref as tr
from sweep_common import C, F, NAN, SENTINEL, Ck, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                 # include/hypad.h
ONE_PASS = 4 * 4096                                                       # rows of one grid pass: WAVES * wave_grid's cap
# name: (restatement, operand keys of _data)
OPS = {
    "mobius_sub": (gr.mobius_sub_ref, ("x", "y")),
    "mobius_coadd": (gr.mobius_coadd_ref, ("x", "y")),
    "mobius_cosub": (gr.mobius_cosub_ref, ("x", "y")),
    "geodesic_unit": (gr.geodesic_unit_ref, ("t", "x", "u")),
    "lambda_x": (gr.lambda_x_ref, ("x",)),
    "inner": (gr.inner_ref, ("x", "u", "v")),
    "norm": (gr.norm_ref, ("x", "u")),
    "egrad2rgrad": (gr.egrad2rgrad_ref, ("x", "v")),
    "sproj": (gr.sproj_ref, ("h",)),
    "inv_sproj": (gr.inv_sproj_ref, ("x",)),
}
PER_ROW = ("lambda_x", "inner", "norm")                                   # one value per row for the result and grad_out
PROJECTIONS = ("sproj", "inv_sproj")
SHAPES = [(1, 5), (4, 5), (5, 5), (7, 1), (7, 63), (7, 64), (7, 65), (7, 255), (7, 256)]
BALL_WIDTHS = [1, 63, 64, 255]


def _C():
    from hypad_amd import _C as c
    return c


def _gmath():
    from hypad_amd.hyperspace import gmath
    return gmath


def _fn(name):
    gm = _gmath()
    return lambda *ops: getattr(gm, name)(*ops, k=-1.0)


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\ngyro ops {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _equal(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def _unit(g, rows, D):
    a = torch.randn(rows, D, generator=g, dtype=F64)
    return a / a.norm(dim=1, keepdim=True).clamp_min(1e-300)


def _with_h(d):
    d["h"] = gr.inv_sproj_ref(d["y"].double()).float()
    return d


def _data(rows, D, seed=0, radius=0.9):
    """The operands at ball width D, and grad_out by the shape of the result: "row" (rows, D), "per_row" (rows), "wide" (rows, D + 1)."""
    g = torch.Generator().manual_seed(7919 * rows + 31 * D + seed)
    x, y = (_unit(g, rows, D) * torch.rand(rows, 1, generator=g, dtype=F64) * radius for _ in range(2))
    u, v = (_unit(g, rows, D) * (0.1 + 1.4 * torch.rand(rows, 1, generator=g, dtype=F64)) for _ in range(2))
    t = 0.1 + 2.9 * torch.rand(rows, 1, generator=g, dtype=F64)
    go = dict(row=torch.randn(rows, D, generator=g), per_row=torch.randn(rows, generator=g), wide=torch.randn(rows, D + 1, generator=g))
    return _with_h(dict(x=x.float(), y=y.float(), u=u.float(), v=v.float(), t=t.float())), go


def _go(name, go):
    return go["per_row" if name in PER_ROW else "wide" if name == "inv_sproj" else "row"]


def _special(D=5):
    """Row 0: x == y; row 1: zero in both; rows 2 and 3: x and y on the 1 - 1e-3 norm; row 4: a zero tangent u; rows 5, 6, 7: t = 0, -1, 40;
    row 8: none of these."""
    d, go = _data(9, D, seed=5)
    x, y = d["x"].double(), d["y"].double()
    x[2] *= (1 - 1e-3) / x[2].norm()
    y[3] *= (1 - 1e-3) / y[3].norm()
    d["x"], d["y"] = x.float(), y.float()
    d["y"][0] = d["x"][0]
    d["x"][1] = d["y"][1] = 0.0
    d["u"][4] = 0.0
    d["t"][5], d["t"][6], d["t"][7] = 0.0, -1.0, 40.0
    return _with_h(d), go


_REFS = {}


def _refs(name, ops, go, key=None):
    """[out, grads...] of the restatement in fp64 and fp32 (computed once per key)."""
    if key is not None and (name, key) in _REFS:
        return _REFS[(name, key)]
    res = {}
    for dt in (F64, F32):
        leaves = [_leaf(t, dt) for t in ops]
        o = OPS[name][0](*leaves)
        res[dt] = [o.detach()] + list(torch.autograd.grad(o, leaves, go.to(dt)))
    if key is not None:
        _REFS[(name, key)] = res
    return res


def _run(name, ops, go, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    leaves = [mk(t).requires_grad_(True) for t in ops]
    out = _fn(name)(*leaves)
    out.backward(go.cuda())
    return [out.detach()] + [t.grad for t in leaves]


def _check(ck, name, res, got):
    labels = ["out"] + ["grad_" + k for k in OPS[name][1]]
    for lab, t, r64, r32 in zip(labels, got, res[F64], res[F32]):
        assert t.shape == r64.shape, (ck.case, name, lab, t.shape)
        assert bool(torch.isfinite(t).all()), (ck.case, name, lab)
        ck.cmp(f"{name} {lab}", t.cpu(), r64, r32)


def _case(name, d, go, tag, key=None):
    ops = [d[k] for k in OPS[name][1]]
    ck = Ck(f"{name} {tag}")
    _check(ck, name, _refs(name, ops, _go(name, go), key), _run(name, ops, _go(name, go)))
    return ck


# ================================================================================================ the sweep
@pytest.mark.parametrize("rows,D", SHAPES, ids=lambda v: str(v))
def test_every_function_forward_and_backward(rows, D):
    """(The projections have ball width D and hyperboloid width D + 1 here, so they sit out D = 256: their widths are the next test's.)"""
    d, go = _data(rows, D)
    cks = [_case(name, d, go, (rows, D)) for name in OPS if D < 256 or name not in PROJECTIONS]
    _report((rows, D), cks)
    _finish(cks)


@pytest.mark.parametrize("D", BALL_WIDTHS)
def test_projections_at_the_lane_edges_of_their_two_widths(D):
    d, go = _data(7, D, seed=2)
    cks = [_case(name, d, go, f"ball width {D}") for name in PROJECTIONS]
    got = _run("inv_sproj", [d["x"]], go["wide"])[0]
    assert got.shape == (7, D + 1) and _run("sproj", [d["h"]], go["row"])[0].shape == (7, D)
    _report(f"projections, ball width {D}", cks)
    _finish(cks)


_LONG = {}


def _long_results():
    """The 16 385-row case of every function, run twice (with another history of the allocator's blocks in between), computed once."""
    if not _LONG:
        d, go = _data(ONE_PASS + 1, 5)
        for name in OPS:
            ops = [d[k] for k in OPS[name][1]]
            first = _run(name, ops, _go(name, go))
            torch.full((ONE_PASS * 7,), NAN, device="cuda")
            _LONG[name] = (ops, _go(name, go), first, _run(name, ops, _go(name, go)))
    return _LONG


def test_one_row_past_a_grid_pass():
    cks = []
    for name, (ops, go, first, _) in _long_results().items():
        ck = Ck(f"{name} ({ONE_PASS + 1}, 5)")
        _check(ck, name, _refs(name, ops, go), first)
        cks.append(ck)
    _report((ONE_PASS + 1, 5), cks)
    _finish(cks)


def test_two_runs_give_the_same_bits():
    for name, (_, _, first, second) in _long_results().items():
        _equal(first, second, name)


def test_special_rows():
    """x == y, both operands zero, the 1 - 1e-3 norm, a zero tangent, t = 0, -1 and 40: finite, and under the rule against the restatement."""
    d, go = _special()
    cks = [_case(name, d, go, "special rows") for name in OPS]
    sub = _run("mobius_sub", [d["x"], d["y"]], go["row"])[0]
    assert float(sub[:2].abs().max()) <= 1e-7                       # x (-) x = 0 up to the rounding of x (+) (-x)
    nrm = _run("norm", [d["x"], d["u"]], go["per_row"])
    assert float(nrm[0][4]) == 0.0 and float(nrm[2][4].abs().max()) == 0.0 and float(nrm[1][4].abs().max()) == 0.0     # a zero tangent: gradient 0
    geo = _run("geodesic_unit", [d["t"], d["x"], d["u"]], go["row"])
    assert torch.equal(geo[0][4], d["x"][4].cuda()) and torch.equal(geo[0][5], d["x"][5].cuda())      # a zero tangent, t = 0: x itself
    assert abs(float(geo[0][7].double().norm()) - 1.0) <= 1e-6 and float(geo[1][7]) == 0.0            # t = 40: the clamp holds, no dL/dt
    _report("special rows", cks)
    _finish(cks)


def test_recorded_cases_through_the_public_functions():
    from test_gyro_ops_host import CASES, ROW_TBIG, grad_output, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    cks = []
    assert set(CASES) == set(OPS)
    for name, (_, _, _, keys, gk) in CASES.items():
        ops = [fx[k] for k in keys]
        assert tuple(keys) == OPS[name][1]
        lib_shape = fx[f"{name}.out"].shape[:1] if name in PER_ROW else fx[f"{name}.out"].shape      # (inner is recorded with keepdim=True)
        go = grad_output(fx[gk], tuple(lib_shape))
        ck = Ck(f"recorded {name}")
        got = _run(name, ops, go)
        _check(ck, name, _refs(name, ops, go), got)
        if name == "geodesic_unit":
            assert abs(float(got[0][ROW_TBIG].double().norm()) - 1.0) <= 1e-6
        cks.append(ck)
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ identities
def _allow(r64, r32):
    """The rule's absolute allowance for a result whose restatement gives r64 and r32."""
    scale = max(1.0, float(r64.abs().max()))
    return (C * float((r32.double() - r64).abs().max()) / scale + F) * scale


def _sides(fn, ops):
    """(fp64, fp32) of a restated expression."""
    return tuple(fn(*[t.to(dt) for t in ops]) for dt in (F64, F32))


def _same(what, a, b, sides_a, sides_b):
    allow = _allow(*sides_a) + _allow(*sides_b)
    err = float((a.double().cpu() - b.double().cpu()).abs().max())
    print(f"\ngyro ops identity {what}: difference / allowance {err / allow:.3f}")
    assert a.shape == b.shape and err <= allow, (what, err, allow)


@pytest.mark.parametrize("rows,D", [(33, 5), (9, 100)])
def test_identities(rows, D):
    from dist_ref import dist_ref
    gm = _gmath()
    K = dict(k=-1.0)
    d, go = _data(rows, D, seed=3, radius=0.8)
    x, y, u, v, t, g = d["x"], d["y"], d["u"], d["v"], d["t"], go["row"]
    xd, yd, ud, vd, td, gd = (a.cuda() for a in (x, y, u, v, t, g))
    ident = lambda *a: a[-1]
    _same("mobius_cosub(mobius_add(x, y), y) = x", gm.mobius_cosub(gm.mobius_add(xd, yd), yd, **K), xd,
          _sides(lambda a, b: gr.mobius_cosub_ref(tr.mobius_add_ref(a, b), b), (x, y)), _sides(ident, (x,)))
    _same("mobius_coadd(mobius_sub(x, y), y) = x", gm.mobius_coadd(gm.mobius_sub(xd, yd, **K), yd, **K), xd,
          _sides(lambda a, b: gr.mobius_coadd_ref(gr.mobius_sub_ref(a, b), b), (x, y)), _sides(ident, (x,)))
    _same("mobius_sub(mobius_coadd(x, y), y) = x", gm.mobius_sub(gm.mobius_coadd(xd, yd, **K), yd, **K), xd,
          _sides(lambda a, b: gr.mobius_sub_ref(gr.mobius_coadd_ref(a, b), b), (x, y)), _sides(ident, (x,)))
    _same("mobius_add(mobius_cosub(x, y), y) = x", gm.mobius_add(gm.mobius_cosub(xd, yd, **K), yd), xd,
          _sides(lambda a, b: tr.mobius_add_ref(gr.mobius_cosub_ref(a, b), b), (x, y)), _sides(ident, (x,)))
    _same("mobius_coadd(x, y) = mobius_coadd(y, x)", gm.mobius_coadd(xd, yd, **K), gm.mobius_coadd(yd, xd, **K),
          _sides(gr.mobius_coadd_ref, (x, y)), _sides(gr.mobius_coadd_ref, (y, x)))
    hd = gm.inv_sproj(xd, **K)
    _same("sproj(inv_sproj(x)) = x", gm.sproj(hd, **K), xd, _sides(lambda a: gr.sproj_ref(gr.inv_sproj_ref(a)), (x,)), _sides(ident, (x,)))
    space = lambda h: (h[..., :-1] ** 2).sum(-1) / h[..., -1] ** 2
    time = lambda h: 1 - 1 / h[..., -1] ** 2
    _same("inv_sproj(x) on the hyperboloid: |h[:D]|^2 / h[D]^2 = 1 - 1 / h[D]^2", space(hd), time(hd),
          _sides(lambda a: space(gr.inv_sproj_ref(a)), (x,)), _sides(lambda a: time(gr.inv_sproj_ref(a)), (x,)))
    _same("inner(x, u, u) = norm(x, u)^2", gm.inner(xd, ud, ud, **K), gm.norm(xd, ud, **K) ** 2,
          _sides(lambda a, b: gr.inner_ref(a, b, b), (x, u)), _sides(lambda a, b: gr.norm_ref(a, b) ** 2, (x, u)))
    _same("inner(x, egrad2rgrad(x, g), v) = <g, v>", gm.inner(xd, gm.egrad2rgrad(xd, gd, **K), vd, **K), (gd * vd).sum(-1),
          _sides(lambda a, b, c: gr.inner_ref(a, gr.egrad2rgrad_ref(a, b), c), (x, g, v)), _sides(lambda b, c: (b * c).sum(-1), (g, v)))
    assert float(t.abs().max()) <= 3
    e = gm.geodesic_unit(td, xd, ud, **K)
    _same("dist(x, geodesic_unit(t, x, u)) = |t|", gm.dist(xd, e, **K), td.abs().squeeze(-1),
          _sides(lambda c, a, b: dist_ref(a, gr.geodesic_unit_ref(c, a, b)), (t, x, u)), _sides(lambda c: c.abs().squeeze(-1), (t,)))
    _same("geodesic_unit(t, x, u) = expmap(x, t u / norm(x, u))", e, gm.expmap(xd, td * ud / gm.norm(xd, ud, keepdim=True, **K), **K),
          _sides(gr.geodesic_unit_ref, (t, x, u)), _sides(lambda c, a, b: tr.expmap_ref(a, c * b / gr.norm_ref(a, b, keepdim=True)), (t, x, u)))


# ================================================================================================ the same bits
def _abi_data(name, rows, W):
    """Operands and grad_out for a direct call at row width W: the projections' wider side is W, their ball W - 1."""
    D = W - 1 if name in PROJECTIONS else W
    d, go = _data(rows, D)
    return D, [d[k] for k in OPS[name][1]], _go(name, go)


def _abi_tail(name, rows, D):
    return (rows, D, rows) if name == "geodesic_unit" else (rows, D)


def _abi_bwd(c, name, ops, go, grads, tail):
    c.check(getattr(c.lib, f"hypad_{name}_bwd")(*map(c.ptr, ops), c.ptr(go), *map(c.ptr, grads), *tail, c.stream()), f"{name}_bwd")


def test_operands_at_storage_offset_1_give_the_same_bits():
    d, go = _data(39, 100)
    for name, (_, keys) in OPS.items():
        ops = [d[k] for k in keys]
        _equal(_run(name, ops, _go(name, go)), _run(name, ops, _go(name, go), unaligned=True), name)


def test_each_single_gradient_has_the_bits_of_the_full_run():
    c = _C()
    rows = 39
    for name, (_, keys) in OPS.items():
        D, ops, go = _abi_data(name, rows, 100)
        ops, go = [t.reshape(rows) if k == "t" else t for k, t in zip(keys, ops)], go.cuda()
        ops = [t.cuda() for t in ops]
        n, tail = len(ops), _abi_tail(name, rows, D)
        full = [torch.full(t.shape, NAN, device="cuda") for t in ops]
        _abi_bwd(c, name, ops, go, full, tail)
        assert all(bool(torch.isfinite(t).all()) for t in full), name
        for i in range(n):
            grads = [torch.full(t.shape, NAN, device="cuda") if j == i else None for j, t in enumerate(ops)]
            _abi_bwd(c, name, ops, go, grads, tail)
            assert torch.equal(grads[i], full[i]), (name, keys[i])
        _abi_bwd(c, name, ops, go, [None] * n, tail)                # nothing asked for: nothing to do


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    cks = []
    for rows, W in ((5, 65), (7, 256)):
        for name, (_, keys) in OPS.items():
            D, ops, go = _abi_data(name, rows, W)
            res = _refs(name, ops, go, ("guarded", rows, W))
            dev = [(t.reshape(rows) if k == "t" else t).cuda() for k, t in zip(keys, ops)]
            shapes = [tuple(go.shape)] + [tuple(t.shape) for t in dev]
            bufs = [_guarded(s, o) for s, o in zip(shapes, (3, 1, 2, 5))]
            views = [v for _, v in bufs]
            tail = _abi_tail(name, rows, D)
            c.check(getattr(c.lib, f"hypad_{name}_fwd")(*map(c.ptr, dev), c.ptr(views[0]), *tail, c.stream()), f"{name}_fwd")
            _abi_bwd(c, name, dev, go.cuda(), views[1:], tail)
            torch.cuda.synchronize()
            for (buf, _), off in zip(bufs, (3, 1, 2, 5)):
                assert _guards_intact(buf, off), name
            ck = Ck(f"guarded {name} {(rows, W)}")
            _check(ck, name, res, [views[0]] + [v.reshape(r.shape) for v, r in zip(views[1:], res[F64][1:])])
            cks.append(ck)
    _report("between guards", cks)
    _finish(cks)


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    rows = 6
    for D in (257, 256, 8):
        a = torch.zeros(rows, D + 1, device="cuda")
        outs = [torch.full((rows, D + 1), SENTINEL, device="cuda") for _ in range(4)]
        o, g1, g2, g3 = (c.ptr(t) for t in outs)
        p = c.ptr(a)
        for name, (_, keys) in OPS.items():
            n = len(keys)
            fwd, bwd = getattr(L, f"hypad_{name}_fwd"), getattr(L, f"hypad_{name}_bwd")
            geo = name == "geodesic_unit"
            f = lambda ops=(p,) * n, out=o, r=rows, d=D, tc=rows: fwd(*ops, out, r, d, *((tc,) if geo else ()), c.stream())
            b = lambda ops=(p,) * n, go=p, r=rows, d=D, tc=rows: bwd(*ops, go, *(g1, g2, g3)[:n], r, d, *((tc,) if geo else ()), c.stream())
            if D == 257 or (D == 256 and name in PROJECTIONS):      # (the projections' wider side is D + 1)
                assert f() == b() == HYPAD_EUNSUPPORTED, name
                continue
            if D == 256:
                continue
            for i in range(n):
                ops = tuple(None if j == i else p for j in range(n))
                assert f(ops=ops) == b(ops=ops) == HYPAD_EINVAL, (name, i)
            assert f(out=None) == b(go=None) == f(r=-1) == b(r=-2) == f(d=0) == b(d=-1) == HYPAD_EINVAL, name
            if geo:
                assert f(tc=2) == b(tc=0) == f(tc=-1) == HYPAD_EINVAL
            assert f(ops=(None,) * n, out=None, r=0, tc=0) == b(ops=(None,) * n, go=None, r=0, tc=0) == 0, name       # no rows: nothing is launched
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == SENTINEL).all())                  # nothing ran
    gm = _gmath()
    with pytest.raises(NotImplementedError, match="supported"):
        gm.mobius_sub(torch.zeros(2, 257, device="cuda"), torch.zeros(2, 257, device="cuda"), k=-1.0)
    with pytest.raises(NotImplementedError, match="supported"):
        gm.inv_sproj(torch.zeros(2, 256, device="cuda"), k=-1.0)
    e = torch.zeros(2, 0, 8, device="cuda", requires_grad=True)     # no rows: the shapes go through, nothing is launched
    out = gm.mobius_coadd(e, e, k=-1.0)
    out.sum().backward()
    s = gm.inner(e, e, e, k=-1.0)
    h = gm.inv_sproj(e, k=-1.0)
    assert out.shape == (2, 0, 8) and e.grad.shape == (2, 0, 8) and s.shape == (2, 0) and h.shape == (2, 0, 9) and gm.sproj(h, k=-1.0).shape == (2, 0, 8)


# ================================================================================================ broadcasting
def test_broadcast_operands_and_a_shared_t():
    gm = _gmath()
    g = torch.Generator().manual_seed(1226)
    cen = (_unit(g, 2, 5) * 0.5).float().reshape(2, 1, 5)
    xs = (_unit(g, 18, 5) * torch.rand(18, 1, generator=g, dtype=F64) * 0.9).float().reshape(2, 9, 5)
    go, gs = torch.randn(2, 9, 5, generator=g), torch.randn(2, 9, generator=g)
    res = {}
    for dt in (F64, F32):
        cc, xx, tt = _leaf(cen, dt), _leaf(xs, dt), _leaf(torch.tensor(0.7), dt)
        sb = gr.mobius_sub_ref(cc, xx)
        ge = gr.geodesic_unit_ref(tt, cc, xx)
        inn = gr.inner_ref(cc, xx, xx * 0.5 + 1.0)
        res[dt] = ([sb.detach()] + list(torch.autograd.grad(sb, [cc, xx], go.to(dt))), [ge.detach()] + list(torch.autograd.grad(ge, [tt, cc, xx], go.to(dt))),
                   [inn.detach()] + list(torch.autograd.grad(inn, [cc, xx], gs.to(dt))))
    cd, xd, td = cen.cuda().requires_grad_(True), xs.cuda().requires_grad_(True), torch.tensor(0.7, device="cuda", requires_grad=True)
    sb = gm.mobius_sub(cd, xd, k=-1.0)
    got_sb = [sb.detach()] + list(torch.autograd.grad(sb, [cd, xd], go.cuda()))
    ge = gm.geodesic_unit(td, cd, xd, k=-1.0)
    got_ge = [ge.detach()] + list(torch.autograd.grad(ge, [td, cd, xd], go.cuda()))
    inn = gm.inner(cd, xd, xd * 0.5 + 1.0, k=-1.0)                   # (x broadcast; xs is in both tangents: its two gradients are added)
    got_in = [inn.detach()] + list(torch.autograd.grad(inn, [cd, xd], gs.cuda()))
    assert sb.shape == ge.shape == (2, 9, 5) and inn.shape == (2, 9) and got_sb[1].shape == got_in[1].shape == (2, 1, 5) and got_ge[1].shape == ()
    ck = Ck("broadcast (2, 1, 5) against (2, 9, 5)")
    for what, got, i in (("mobius_sub", got_sb, 0), ("geodesic_unit, shared t", got_ge, 1), ("inner, broadcast x", got_in, 2)):
        for j, t in enumerate(got):
            ck.cmp(f"{what} tensor {j}", t.cpu(), res[F64][i][j], res[F32][i][j])
    assert torch.equal(gm.geodesic_unit(0.7, cd, xd, k=-1.0), ge.detach())       # a number is the one-element tensor
    trow = torch.full((2, 9, 1), 0.7, device="cuda", requires_grad=True)          # ... and one value per row: the same points, its gradient per row
    gr_ = gm.geodesic_unit(trow, cd, xd, k=-1.0)
    assert torch.equal(gr_.detach(), ge.detach())
    (gt,) = torch.autograd.grad(gr_, [trow], go.cuda())
    assert gt.shape == (2, 9, 1)
    ck.cmp("geodesic_unit, sum of the per-row grad_t", gt.double().sum().cpu(), res[F64][1][1], res[F32][1][1])
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ side stream, captured graph
def _stream_cases():
    d, go = _data(39, 100)
    gm = _gmath()
    return [("mobius_sub", (d["x"], d["y"], go["row"]), lambda a, b: gm.mobius_sub(a, b, k=-1.0)),
            ("inner", (d["x"], d["u"], go["per_row"]), lambda a, b: gm.inner(a, b, a * 0.5 + b, k=-1.0))]


def _fwd_bwd(fn, a, b, go):
    out = fn(a, b)
    ga, gb = torch.autograd.grad(out, [a, b], go)
    return out, ga, gb


def test_on_a_side_stream():
    for name, host, fn in _stream_cases():
        a, b, go = (t.cuda() for t in host)
        want = [t.clone() for t in _fwd_bwd(fn, a.requires_grad_(True), b.requires_grad_(True), go)]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            a2, b2, go2 = (t.cuda() for t in host)          # placed and filled on the side stream: a launch on stream 0 would race them
            got = _fwd_bwd(fn, a2.requires_grad_(True), b2.requires_grad_(True), go2)
        side.synchronize()
        _equal(got, want, name + " on a side stream")


def test_captured_and_replayed_with_changed_inputs():
    for name, host, fn in _stream_cases():
        g = torch.Generator().manual_seed(11)
        second = (host[0].flip(0).contiguous(), (host[1] * 0.5).contiguous(), torch.randn(host[2].shape, generator=g))
        wants = []
        for h in (host, second):
            a, b, go = (t.cuda() for t in h)
            wants.append([t.clone() for t in _fwd_bwd(fn, a.requires_grad_(True), b.requires_grad_(True), go)])
        assert not torch.equal(wants[0][0], wants[1][0])
        static = [t.cuda() for t in host]
        static[0].requires_grad_(True), static[1].requires_grad_(True)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            _fwd_bwd(fn, *static)                           # the eager warm-up, on the capture stream
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            outs = _fwd_bwd(fn, *static)
        for i in (1, 0):                                    # replayed twice, each time with other inputs
            with torch.no_grad():
                for s, h in zip(static, (host, second)[i]):
                    s.copy_(h.cuda())
            graph.replay()
            torch.cuda.synchronize()
            _equal([t.detach() for t in outs], wants[i], f"{name} replay with data set {i}")


# ================================================================================================ the chain
def test_hand_written_riemannian_gradient_descent():
    """Five steps of Riemannian gradient descent on the rows of a (6, 20) ball parameter -- the shape class of MobiusDist2Hyperplane.point --
    towards fixed targets: loss = sum of dist, step = egrad2rgrad(p, grad), p <- expmap(p, -lr step).  A step moves a row by lr along its
    geodesic to the target, so the loss falls by about 6 lr a step.  Against the same loop of the restatement, steps = 5."""
    from dist_ref import dist_ref
    rows, D, steps, lr = 6, 20, 5, 0.1
    g = torch.Generator().manual_seed(20)
    p0 = (_unit(g, rows, D) * (0.3 + 0.5 * torch.rand(rows, 1, generator=g, dtype=F64))).float()
    target = (_unit(g, rows, D) * (0.3 + 0.5 * torch.rand(rows, 1, generator=g, dtype=F64))).float()
    res = {}
    for dt in (F64, F32):
        p, tg, losses = p0.to(dt), target.to(dt), []
        for _ in range(steps):
            p = p.detach().requires_grad_(True)
            loss = dist_ref(p, tg).sum()
            (grad,) = torch.autograd.grad(loss, [p])
            losses.append(loss.detach())
            p = tr.expmap_ref(p.detach(), -lr * gr.egrad2rgrad_ref(p.detach(), grad))
        res[dt] = dict(p=p.detach(), losses=torch.stack(losses + [dist_ref(p, tg).sum().detach()]))
    gm = _gmath()
    p, tg, losses = p0.cuda(), target.cuda(), []
    for _ in range(steps):
        p = p.detach().requires_grad_(True)
        loss = gm.dist(p, tg, k=-1.0).sum()
        (grad,) = torch.autograd.grad(loss, [p])
        losses.append(loss.detach())
        with torch.no_grad():
            p = gm.expmap(p.detach(), -lr * gm.egrad2rgrad(p.detach(), grad, k=-1.0), k=-1.0)
    losses = torch.stack(losses + [gm.dist(p, tg, k=-1.0).sum()])
    ck = Ck(f"Riemannian gradient descent {(rows, D)}, {steps} steps")
    ck.cmp("p", p.cpu(), res[F64]["p"], res[F32]["p"], steps=steps)
    ck.cmp("losses", losses.cpu(), res[F64]["losses"], res[F32]["losses"], steps=steps)
    assert float(p.norm(dim=-1).max()) < 1.0 and bool(torch.isfinite(p).all())
    assert float(losses[-1]) < float(losses[0]) - 0.5 * steps * lr * rows, losses.tolist()
    _report(ck.case, [ck])
    _finish([ck])
