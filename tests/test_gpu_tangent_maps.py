"""The tangent maps expmap, logmap, geodesic, gyration, parallel_transport, parallel_transport0 and parallel_transport0back on the GPU
(hypad_<name>_fwd / _bwd of csrc/tangent.hip; hyperspace/gmath runs them) against the plain-torch restatement of tests/tangent_ref.py
-- which tests/test_tangent_maps_host.py pins to the reference's own outputs -- run in fp64 and fp32 on the CPU, under the project's
rule ``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1).  No tolerance of its own.

The data (``_data``).  Points x and y within radius 0.9, a tangent u with norms up to 1.5, t (rows, 1) in [0.1, 0.9], grad_out ~ N(0, 1).
The special rows get tests of their own and do not set err32 for the others: x == y at norms 0.3 and 0.6, both operands zero, a zero
tangent, a point on the 1 - 1e-3 norm.

The kernels have no tile: a wave per row, 64 lanes x 4 elements, four waves a workgroup, at most 4 096 workgroups a launch.  So the
shapes are rows 1, 4 and 5 (a workgroup's waves not filled, filled, one past), 16 385 = 4 * 4 096 + 1 (one row past a single grid pass)
and D = 1, 63, 64, 65, 255, 256 (one to four elements a lane, the last lane empty or full).

The identities compare two results of the library with each other; each side is off its own fp64 value by at most the rule's
allowance for it (C * err32 + F with the restatement's err32 for that side), so the two may differ by the sum of the two allowances.
"""
import pytest
import torch

import tangent_ref as tr
from sweep_common import C, F, NAN, SENTINEL, Ck, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                 # include/hypad.h
ONE_PASS = 4 * 4096                                                       # rows of one grid pass: WAVES * wave_grid's cap
# name: (restatement, operand keys of _data)
OPS = {
    "expmap": (tr.expmap_ref, ("x", "u")),
    "logmap": (tr.logmap_ref, ("x", "y")),
    "geodesic": (tr.geodesic_ref, ("t", "x", "y")),
    "gyration": (tr.gyration_ref, ("x", "y", "u")),
    "parallel_transport": (tr.parallel_transport_ref, ("x", "y", "u")),
    "parallel_transport0": (tr.parallel_transport0_ref, ("y", "u")),
    "parallel_transport0back": (tr.parallel_transport0back_ref, ("x", "u")),
}
SHAPES = [(1, 5), (4, 5), (5, 5), (7, 1), (7, 63), (7, 64), (7, 65), (7, 255), (7, 256)]


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
    print(f"\ntangent maps {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _equal(a, b, what):
    assert len(a) == len(b)
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def _unit(g, rows, D):
    a = torch.randn(rows, D, generator=g, dtype=F64)
    return a / a.norm(dim=1, keepdim=True).clamp_min(1e-300)


def _data(rows, D, seed=0, radius=0.9):
    g = torch.Generator().manual_seed(7919 * rows + 31 * D + seed)
    x, y, u = (_unit(g, rows, D) * torch.rand(rows, 1, generator=g, dtype=F64) * s for s in (radius, radius, 1.5))
    t = 0.1 + 0.8 * torch.rand(rows, 1, generator=g, dtype=F64)
    return dict(x=x.float(), y=y.float(), u=u.float(), t=t.float()), torch.randn(rows, D, generator=g)


def _special(D=5):
    """Rows 0 and 1: x == y at norms 0.3 and 0.6; row 2: zero in both; row 3: a zero tangent; row 4: x on the 1 - 1e-3 norm; row 5: y
    there; row 6: t = 0; row 7: t = 1; row 8: a tangent of norm 12 from |x| = 0.6 (the tanh clamp)."""
    d, go = _data(9, D, seed=5)
    x, y, u, t = d["x"].double(), d["y"].double(), d["u"].double(), d["t"]
    x[0] *= 0.3 / x[0].norm()
    x[1] *= 0.6 / x[1].norm()
    x[4] *= (1 - 1e-3) / x[4].norm()
    y[5] *= (1 - 1e-3) / y[5].norm()
    x[8] *= 0.6 / x[8].norm()
    u[8] *= 12 / u[8].norm()
    x, y, u = x.float(), y.float(), u.float()
    y[0], y[1] = x[0], x[1]
    x[2] = y[2] = 0.0
    u[3] = 0.0
    t[6], t[7] = 0.0, 1.0
    return dict(x=x, y=y, u=u, t=t), go


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
    _check(ck, name, _refs(name, ops, go, key), _run(name, ops, go))
    return ck


# ================================================================================================ the sweep
@pytest.mark.parametrize("rows,D", SHAPES, ids=lambda v: str(v))
def test_every_map_forward_and_backward(rows, D):
    d, go = _data(rows, D)
    cks = [_case(name, d, go, (rows, D)) for name in OPS]
    _report((rows, D), cks)
    _finish(cks)


_LONG = {}


def _long_results():
    """The 16 385-row case of every map, run twice (with another history of the allocator's blocks in between), computed once."""
    if not _LONG:
        d, go = _data(ONE_PASS + 1, 5)
        for name in OPS:
            ops = [d[k] for k in OPS[name][1]]
            first = _run(name, ops, go)
            torch.full((ONE_PASS * 7,), NAN, device="cuda")
            _LONG[name] = (ops, go, first, _run(name, ops, go))
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
    """x == y at norms 0.3 and 0.6, both operands zero, a zero tangent, the 1 - 1e-3 norm, t = 0 and 1, the tanh clamp: finite, and under
    the rule against the restatement, whose log1p artanh follows the same limit at coincident points."""
    d, go = _special()
    cks = [_case(name, d, go, "special rows") for name in OPS]
    got = _run("logmap", [d["x"], d["y"]], go)
    assert float(got[0][:3].abs().max()) <= 1e-7                    # log_x(x) = 0 up to the rounding of (-x) (+) x
    got = _run("geodesic", [d["t"], d["x"], d["y"]], go)
    assert float((got[0][:3] - d["x"][:3].cuda()).abs().max()) <= 1e-7
    _report("special rows", cks)
    _finish(cks)


def test_recorded_cases_through_the_public_functions():
    from test_tangent_maps_host import CASES, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    cks = []
    assert set(CASES) == set(OPS)
    for name, (_, _, _, keys) in CASES.items():
        ops = [fx[k] for k in keys]
        ck = Ck(f"recorded {name}")
        _check(ck, name, _refs(name, ops, fx["grad_output"]), _run(name, ops, fx["grad_output"]))
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
    err = float((a.double() - b.double()).abs().max())
    print(f"\ntangent maps identity {what}: difference / allowance {err / allow:.3f}")
    assert err <= allow, (what, err, allow)


@pytest.mark.parametrize("rows,D", [(33, 5), (9, 100)])
def test_identities(rows, D):
    gm = _gmath()
    d, _ = _data(rows, D, seed=3, radius=0.8)
    x, y, v, t = d["x"], d["y"], d["u"], d["t"]
    lam = 2 / (1 - x.double().pow(2).sum(-1, keepdim=True))
    u = (v.double() * torch.clamp(3 / (lam * v.double().norm(dim=-1, keepdim=True)), max=1.0)).float()      # lambda_x |u| <= 3
    xd, yd, ud, vd = x.cuda(), y.cuda(), u.cuda(), v.cuda()
    ident = lambda *a: a[-1]
    e = gm.expmap(xd, ud, k=-1.0)
    _same("logmap(x, expmap(x, u)) = u", gm.logmap(xd, e, k=-1.0).cpu(), u, _sides(lambda a, b: tr.logmap_ref(a, tr.expmap_ref(a, b)), (x, u)),
          _sides(ident, (u,)))
    lam_u = lambda a, b: (tr._lambda(a) * tr._norm(b)).squeeze(-1)
    from dist_ref import dist_ref
    _same("dist(x, expmap(x, u)) = lambda_x |u|", gm.dist(xd, e, k=-1.0).cpu(), lam_u(x.double(), u.double()),
          _sides(lambda a, b: dist_ref(a, tr.expmap_ref(a, b)), (x, u)), _sides(lam_u, (x, u)))
    for tv, end, what in ((0.0, x, "geodesic(0, x, y) = x"), (1.0, y, "geodesic(1, x, y) = y")):
        _same(what, gm.geodesic(tv, xd, yd, k=-1.0).cpu(), end, _sides(lambda a, b: tr.geodesic_ref(torch.tensor(tv, dtype=a.dtype), a, b), (x, y)),
              _sides(ident, (end,)))
    lam_v = lambda p, w: (tr._lambda(p) * tr._norm(w)).squeeze(-1)
    pt = gm.parallel_transport(xd, yd, vd, k=-1.0)
    _same("lambda_y |parallel_transport(x, y, v)| = lambda_x |v|", lam_v(yd, pt).cpu(), lam_v(x.double(), v.double()),
          _sides(lambda a, b, c: lam_v(b, tr.parallel_transport_ref(a, b, c)), (x, y, v)), _sides(lam_v, (x, v)))
    zero = torch.zeros_like(x)
    _same("parallel_transport(0, y, v) = parallel_transport0(y, v)", gm.parallel_transport(zero.cuda(), yd, vd, k=-1.0).cpu(),
          gm.parallel_transport0(yd, vd, k=-1.0).cpu(), _sides(lambda b, c: tr.parallel_transport_ref(torch.zeros_like(b), b, c), (y, v)),
          _sides(tr.parallel_transport0_ref, (y, v)))
    _same("parallel_transport0back(x, parallel_transport0(x, v)) = v", gm.parallel_transport0back(xd, gm.parallel_transport0(xd, vd, k=-1.0), k=-1.0).cpu(), v,
          _sides(lambda a, c: tr.parallel_transport0back_ref(a, tr.parallel_transport0_ref(a, c)), (x, v)), _sides(ident, (v,)))


# ================================================================================================ the same bits
def test_operands_at_storage_offset_1_give_the_same_bits():
    d, go = _data(39, 100)
    for name, (_, keys) in OPS.items():
        ops = [d[k] for k in keys]
        _equal(_run(name, ops, go), _run(name, ops, go, unaligned=True), name)


def _abi_bwd(c, name, ops, go, grads, tcount=None):
    rows, D = go.shape
    tail = (rows, D) if tcount is None else (rows, D, tcount)
    c.check(getattr(c.lib, f"hypad_{name}_bwd")(*map(c.ptr, ops), c.ptr(go), *map(c.ptr, grads), *tail, c.stream()), f"{name}_bwd")


def test_each_single_gradient_has_the_bits_of_the_full_run():
    c = _C()
    rows, D = 39, 100
    d, go = _data(rows, D)
    go = go.cuda()
    for name, (_, keys) in OPS.items():
        ops = [d[k].cuda() for k in keys]
        n = len(ops)
        shapes = [(rows,) if k == "t" else (rows, D) for k in keys]
        tcount = rows if name == "geodesic" else None
        full = [torch.full(s, NAN, device="cuda") for s in shapes]
        _abi_bwd(c, name, ops, go, full, tcount)
        assert all(bool(torch.isfinite(t).all()) for t in full), name
        for i in range(n):
            grads = [torch.full(s, NAN, device="cuda") if j == i else None for j, s in enumerate(shapes)]
            _abi_bwd(c, name, ops, go, grads, tcount)
            assert torch.equal(grads[i], full[i]), (name, keys[i])
        _abi_bwd(c, name, ops, go, [None] * n, tcount)              # nothing asked for: nothing to do


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    cks = []
    for rows, D in ((5, 65), (7, 256)):
        d, go = _data(rows, D)
        for name, (_, keys) in OPS.items():
            ops = [d[k] for k in keys]
            res = _refs(name, ops, go, (rows, D))
            dev = [t.cuda() for t in ops]
            shapes = [(rows, D)] + [(rows,) if k == "t" else (rows, D) for k in keys]
            bufs = [_guarded(s, o) for s, o in zip(shapes, (3, 1, 2, 5))]
            views = [v for _, v in bufs]
            tail = (rows, D, rows) if name == "geodesic" else (rows, D)
            c.check(getattr(c.lib, f"hypad_{name}_fwd")(*map(c.ptr, dev), c.ptr(views[0]), *tail, c.stream()), f"{name}_fwd")
            _abi_bwd(c, name, dev, go.cuda(), views[1:], rows if name == "geodesic" else None)
            torch.cuda.synchronize()
            for (buf, _), off in zip(bufs, (3, 1, 2, 5)):
                assert _guards_intact(buf, off), name
            ck = Ck(f"guarded {name} {(rows, D)}")
            _check(ck, name, res, [views[0]] + [v.reshape(r.shape) for v, r in zip(views[1:], res[F64][1:])])
            cks.append(ck)
    _report("between guards", cks)
    _finish(cks)


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    rows = 6
    for D in (257, 8):
        a = torch.zeros(rows, D, device="cuda")
        outs = [torch.full((rows, D), SENTINEL, device="cuda") for _ in range(4)]
        o, g1, g2, g3 = (c.ptr(t) for t in outs)
        p = c.ptr(a)
        for name, (_, keys) in OPS.items():
            n = len(keys)
            fwd, bwd = getattr(L, f"hypad_{name}_fwd"), getattr(L, f"hypad_{name}_bwd")
            geo = name == "geodesic"
            f = lambda ops=(p,) * n, out=o, r=rows, d=D, tc=rows: fwd(*ops, out, r, d, *((tc,) if geo else ()), c.stream())
            b = lambda ops=(p,) * n, go=p, r=rows, d=D, tc=rows: bwd(*ops, go, *(g1, g2, g3)[:n], r, d, *((tc,) if geo else ()), c.stream())
            if D == 257:
                assert f() == b() == HYPAD_EUNSUPPORTED, name
                continue
            for i in range(n):
                ops = tuple(None if j == i else p for j in range(n))
                assert f(ops=ops) == b(ops=ops) == HYPAD_EINVAL, (name, i)
            assert f(out=None) == b(go=None) == f(r=-1) == b(r=-2) == f(d=0) == b(d=-1) == HYPAD_EINVAL, name
            if geo:
                assert f(tc=2) == b(tc=0) == f(tc=-1) == HYPAD_EINVAL
        torch.cuda.synchronize()
        for t in outs:
            assert bool((t == SENTINEL).all())                  # nothing ran
    gm = _gmath()
    with pytest.raises(NotImplementedError, match="supported"):
        gm.logmap(torch.zeros(2, 257, device="cuda"), torch.zeros(2, 257, device="cuda"), k=-1.0)
    e = torch.zeros(2, 0, 8, device="cuda", requires_grad=True)     # no rows: the shapes go through, nothing is launched
    out = gm.parallel_transport(e, e, e, k=-1.0)
    out.sum().backward()
    assert out.shape == (2, 0, 8) and e.grad.shape == (2, 0, 8)


# ================================================================================================ broadcasting
def test_broadcast_operands_and_a_shared_t():
    gm = _gmath()
    g = torch.Generator().manual_seed(1226)
    cen = (_unit(g, 2, 5) * 0.5).float().reshape(2, 1, 5)
    xs = (_unit(g, 18, 5) * torch.rand(18, 1, generator=g, dtype=F64) * 0.9).float().reshape(2, 9, 5)
    go = torch.randn(2, 9, 5, generator=g)
    res = {}
    for dt in (F64, F32):
        cc, xx, tt = _leaf(cen, dt), _leaf(xs, dt), _leaf(torch.tensor(0.3), dt)
        lg = tr.logmap_ref(cc, xx)
        ge = tr.geodesic_ref(tt, cc, xx)
        pt = tr.parallel_transport_ref(xx, cc, xx)
        res[dt] = ([lg.detach()] + list(torch.autograd.grad(lg, [cc, xx], go.to(dt))), [ge.detach()] + list(torch.autograd.grad(ge, [tt, cc, xx], go.to(dt))),
                   [pt.detach()] + list(torch.autograd.grad(pt, [cc, xx], go.to(dt))))
    cd, xd, td = cen.cuda().requires_grad_(True), xs.cuda().requires_grad_(True), torch.tensor(0.3, device="cuda", requires_grad=True)
    lg = gm.logmap(cd, xd, k=-1.0)
    got_lg = [lg.detach()] + list(torch.autograd.grad(lg, [cd, xd], go.cuda()))
    ge = gm.geodesic(td, cd, xd, k=-1.0)
    got_ge = [ge.detach()] + list(torch.autograd.grad(ge, [td, cd, xd], go.cuda()))
    pt = gm.parallel_transport(xd, cd, xd, k=-1.0)                  # (x is both the start and the vector: its two gradients are added)
    got_pt = [pt.detach()] + list(torch.autograd.grad(pt, [cd, xd], go.cuda()))
    assert lg.shape == ge.shape == pt.shape == (2, 9, 5) and got_lg[1].shape == (2, 1, 5) and got_ge[1].shape == ()
    ck = Ck("broadcast (2, 1, 5) against (2, 9, 5)")
    for what, got, i in (("logmap", got_lg, 0), ("geodesic, shared t", got_ge, 1), ("parallel_transport", got_pt, 2)):
        for j, t in enumerate(got):
            ck.cmp(f"{what} tensor {j}", t.cpu(), res[F64][i][j], res[F32][i][j])
    assert torch.equal(gm.geodesic(0.3, cd, xd, k=-1.0), ge.detach())       # a number is the one-element tensor
    trow = torch.full((2, 9, 1), 0.3, device="cuda", requires_grad=True)     # ... and one value per row: the same points, its gradient per row
    gr = gm.geodesic(trow, cd, xd, k=-1.0)
    assert torch.equal(gr.detach(), ge.detach())
    (gt,) = torch.autograd.grad(gr, [trow], go.cuda())
    assert gt.shape == (2, 9, 1)
    ck.cmp("geodesic, sum of the per-row grad_t", gt.double().sum().cpu(), res[F64][1][1], res[F32][1][1])
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ side stream, captured graph
def _stream_cases():
    d, go = _data(39, 100)
    gm = _gmath()
    return [("logmap", (d["x"], d["y"], go), lambda a, b: gm.logmap(a, b, k=-1.0)),
            ("parallel_transport", (d["x"], d["y"], go), lambda a, b: gm.parallel_transport(a, b, a * 0.5 + b, k=-1.0))]


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
def test_centroid_tangent_readout_chain():
    """weighted_midpoint centroid -> logmap at it -> parallel_transport0back to the origin's tangent space -> a linear read-out -> a loss:
    every gradient against the same chain in torch (midpoint_ref, tangent_ref)."""
    from midpoint_ref import weighted_midpoint_ref
    B, N, D, H = 3, 9, 20, 4
    g = torch.Generator().manual_seed(19532087)
    xs = (_unit(g, B * N, D) * torch.rand(B * N, 1, generator=g, dtype=F64) * 0.8).float().reshape(B, N, D)
    w, bias, target = torch.randn(H, D, generator=g) / D ** 0.5, 0.1 * torch.randn(H, generator=g), torch.randn(B, N, H, generator=g)
    names = ("xs", "w", "bias")
    res = {}
    for dt in (F64, F32):
        p = {n: _leaf(t, dt) for n, t in zip(names, (xs, w, bias))}
        cen = weighted_midpoint_ref(p["xs"], reducedim=[1], keepdim=True)
        tan = tr.logmap_ref(cen, p["xs"])
        flat = tr.parallel_transport0back_ref(cen, tan)
        loss = ((flat @ p["w"].T + p["bias"] - target.to(dt)) ** 2).mean()
        gs = torch.autograd.grad(loss, [p[n] for n in names])
        res[dt] = dict(cen=cen.detach(), tan=tan.detach(), flat=flat.detach(), loss=loss.detach(), **{"g_" + n: v for n, v in zip(names, gs)})
    gm = _gmath()
    d = {n: t.cuda().requires_grad_(True) for n, t in zip(names, (xs, w, bias))}
    cen = gm.weighted_midpoint(d["xs"], -1.0, reducedim=[1], keepdim=True)
    tan = gm.logmap(cen, d["xs"], k=-1.0)
    flat = gm.parallel_transport0back(cen, tan, k=-1.0)
    loss = ((flat @ d["w"].T + d["bias"] - target.cuda()) ** 2).mean()
    loss.backward()
    ck = Ck(f"centroid chain {(B, N, D)}")
    r64, r32 = res[F64], res[F32]
    for name, t in (("cen", cen.detach()), ("tan", tan.detach()), ("flat", flat.detach()), ("loss", loss.detach()), ("g_xs", d["xs"].grad),
                    ("g_w", d["w"].grad), ("g_bias", d["bias"].grad)):
        assert bool(torch.isfinite(t).all()), name
        ck.cmp(name, t.cpu(), r64[name], r32[name])
    _report(ck.case, [ck])
    _finish([ck])
