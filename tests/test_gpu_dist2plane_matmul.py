"""dist2plane_matmul on the GPU (hypad_dist2plane_matmul_*; hyperspace/gmath runs them) against the plain-torch restatement of
tests/dist2plane_matmul_ref.py -- which tests/test_dist2plane_matmul_host.py pins to the reference's own outputs -- run in fp64 and fp32
on the CPU, under the project's rule ``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1) on out and the three gradients.  No
tolerance of its own and no mask: the formula has no kink apart from its clamps.

The data.  x and the planes' points: ``_ball_rows`` within radius 0.8 (no rim row; the last row of x all zero); normals N(0, 1) scaled to
norms in [0.3, 2], the last one all zero; grad_out ~ N(0, 1).  A point on the 1 - 1e-3 norm moves err32 of every tensor it touches, so it
gets a test of its own per shape -- once as a row of x, once as a point of a plane -- and does not set err32 for the others.

Tile and chunk sizes of the kernels (csrc/dist2plane_matmul.hip), each with a shape at, one below and one above it in ``EDGES``:
    forward: 64 x 64 tiles of out, D in chunks of 128     N (1,63..65,20,20), M (1,20,63..65,20), D (1,20,20,127..129), (1,16,260,256)
    backward: 64 own rows or planes, the other side in chunks of 64 (D <= 128), 32 (grad_x, D > 128) or 16 (the planes, D > 128),
              accumulator classes D <= 64 / 128 / 256     D (1,20,20,63), (1,64,100,64), (1,20,20,65), (1,20,20,127..129), (1,16,260,256)
    65 chunks: (1,17,4099,20) for grad_x, (1,4099,17,20) for grad_p and grad_z
"""
import numpy as np
import pytest
import torch

from dist2plane_matmul_ref import dist2plane_matmul_ref
from sweep_common import C, F, NAN, SENTINEL, Ck, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                 # include/hypad.h
SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (3, 17, 33, 20), (1, 64, 100, 64), (2, 65, 129, 100), (1, 16, 260, 256)]   # (batch, N, M, D)
EDGES = [(1, 63, 20, 20), (1, 65, 20, 20), (1, 20, 63, 20), (1, 20, 64, 20), (1, 20, 65, 20), (1, 20, 20, 63), (1, 20, 20, 65),
         (1, 20, 20, 127), (1, 20, 20, 128), (1, 20, 20, 129)]
LONG = [(1, 17, 4099, 20), (1, 4099, 17, 20)]
NAMES = ("out", "grad_x", "grad_p", "grad_z")
_ids = lambda s: "x".join(map(str, s))


def _C():
    from hypad_amd import _C as c
    return c


def _gmath():
    from hypad_amd.hyperspace import gmath
    return gmath


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\ndist2plane_matmul {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _equal(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def _to_rim(rows2d, g):
    """One row of a (rows, D) matrix moved to the 1 - 1e-3 norm (a zero row gets a direction first)."""
    i = 1 if rows2d.shape[0] >= 3 else 0
    v = rows2d[i].double()
    if float(v.norm()) == 0:
        v = torch.randn(v.shape, generator=g, dtype=F64)
    rows2d[i] = (v * ((1 - 1e-3) / float(v.norm()))).float()


def _data(batch, N, M, D, rim=None, seed=0):
    """x (batch, N, D), the planes' points and normals as rows (batch, M, D), grad_out (batch, N, M)."""
    g = torch.Generator().manual_seed(1000003 * batch + 10007 * N + 101 * M + D + seed)
    x = _ball_rows(g, batch * N, D, edge=False, radius=0.8)
    pp = _ball_rows(g, batch * M, D, edge=False, radius=0.8, zero_row=False)
    zz = torch.randn(batch * M, D, generator=g, dtype=F64)
    zz = (zz / zz.norm(dim=1, keepdim=True) * (0.3 + 1.7 * torch.rand(batch * M, 1, generator=g, dtype=F64))).float()
    if batch * M >= 2:
        zz[-1] = 0.0
    if rim == "x":
        _to_rim(x, g)
    if rim == "p":
        _to_rim(pp, g)
    return x.reshape(batch, N, D), pp.reshape(batch, M, D), zz.reshape(batch, M, D), torch.randn(batch, N, M, generator=g)


_REFS = {}


def _refs(key, x, pp, zz, go):
    """out and the gradients of x and of the rows of the planes, of the restatement in fp64 and fp32 (computed once per key)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        leaves = [_leaf(t, dt) for t in (x, pp, zz)]
        o = dist2plane_matmul_ref(leaves[0], leaves[1].transpose(-1, -2), leaves[2].transpose(-1, -2))
        res[dt] = [o.detach()] + list(torch.autograd.grad(o, leaves, go.to(dt)))
    if key is not None:
        _REFS[key] = res
    return res


def _run(x, pp, zz, go, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, pd, zd = (mk(t).requires_grad_(True) for t in (x, pp, zz))
    out = _gmath().dist2plane_matmul(xd, pd.transpose(-1, -2), zd.transpose(-1, -2), k=-1.0)
    out.backward(go.cuda())
    return out.detach(), xd.grad, pd.grad, zd.grad


def _check(ck, res, got):
    for name, t, r64, r32 in zip(NAMES, got, res[F64], res[F32]):
        assert bool(torch.isfinite(t).all()), (ck.case, name)
        ck.cmp(name, t.cpu(), r64, r32)


def _case(shape, rim=None):
    x, pp, zz, go = _data(*shape, rim=rim)
    ck = Ck(f"{shape}" + (f" rim {rim}" if rim else ""))
    got = _run(x, pp, zz, go)
    _check(ck, _refs((shape, rim), x, pp, zz, go), got)
    if shape[0] * shape[2] >= 2:                            # the zero normal: a zero column of out, nothing to its plane
        assert not got[0][-1, :, -1].any() and not got[2][-1, -1].any() and not got[3][-1, -1].any()
    return ck


@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=_ids)
def test_forward_and_backward(shape):
    ck = _case(shape)
    _report(ck.case, [ck])
    _finish([ck])


@pytest.mark.parametrize("rim", ["x", "p"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_rim_point(shape, rim):
    ck = _case(shape, rim=rim)
    _report(ck.case, [ck])
    _finish([ck])


@pytest.mark.parametrize("shape", LONG, ids=_ids)
def test_walk_of_65_chunks_twice_the_same_bits(shape):
    x, pp, zz, go = _data(*shape)
    got = []
    for _ in range(2):
        got.append(_run(x, pp, zz, go))
        torch.full((4099 * 20 * 7,), NAN, device="cuda")    # (another history of the allocator's blocks between the runs)
    _equal(got[0], got[1], f"{shape}")
    ck = Ck(f"{shape}: 65 chunks")
    _check(ck, _refs(None, x, pp, zz, go), got[0])
    _report(ck.case, [ck])
    _finish([ck])


def test_recorded_case_through_the_public_function():
    from test_dist2plane_matmul_host import ZERO_Z, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    x, p, z, go = fx["x"], fx["p"], fx["z"], fx["grad_output"]
    res = _refs(None, x, p.transpose(-1, -2).contiguous(), z.transpose(-1, -2).contiguous(), go)
    xd, pd, zd = (t.cuda().requires_grad_(True) for t in (x, p, z))     # as recorded: (batch, D, M), materialised
    out = _gmath().dist2plane_matmul(xd, pd, zd, k=torch.tensor(-1.0))
    out.backward(go.cuda())
    got = (out.detach(), xd.grad, pd.grad.transpose(-1, -2), zd.grad.transpose(-1, -2))
    ck = Ck("recorded case")
    _check(ck, res, got)
    ck2 = Ck("recorded case against the reference's own fp64 and fp32 runs")
    for name, t in zip(NAMES, (out.detach(), xd.grad, pd.grad, zd.grad)):
        ck2.cmp(name, t.cpu(), fx["d2pm64." + name], fx["d2pm." + name])
    b, j = ZERO_Z
    assert not out.detach()[b, :, j].any() and not pd.grad[b, :, j].any() and not zd.grad[b, :, j].any()
    _report("recorded case", [ck, ck2])
    _finish([ck, ck2])


def test_batch_dimensions_and_a_side_without_them():
    """Leading batch dimensions (2, 3) on both sides; then x without them and the planes without them: that side is expanded on the host
    and autograd sums its gradient over the batch."""
    x, pp, zz, go = _data(6, 4, 7, 5, seed=3)
    x, pp, zz, go = x.reshape(2, 3, 4, 5), pp.reshape(2, 3, 7, 5), zz.reshape(2, 3, 7, 5), go.reshape(2, 3, 4, 7)
    cks = []
    for tag, x_, p_, z_ in (("both", x, pp, zz), ("x shared", x[0, 0], pp, zz), ("planes shared", x, pp[0, 0], zz[0, 0])):
        res = _refs(None, x_, p_, z_, go)
        got = _run(x_, p_, z_, go)
        assert got[0].shape == (2, 3, 4, 7) and got[1].shape == x_.shape and got[2].shape == p_.shape and got[3].shape == z_.shape
        ck = Ck("batch dims, " + tag)
        _check(ck, res, got)
        cks.append(ck)
    _report("batch dims", cks)
    _finish(cks)


@pytest.mark.parametrize("shape", [(1, 33, 9, 5), (2, 9, 20, 100)], ids=_ids)
def test_identities_on_the_device(shape):
    """The identities of tests/test_dist2plane_matmul_host.py with both sides computed on the device, each held to the sum of the two
    sides' allowances under the rule (each side's fp32 restatement against its fp64 restatement)."""
    from dist2plane_matmul_ref import dist2plane_matmul_bwd
    from test_dist2plane_matmul_host import _data as host_data, identities
    gm = _gmath()
    x, p, z, go = host_data(*shape, seed=7 * shape[1] + shape[3])
    sides = {}
    for dt in (F64, F32):
        a, b, c, g = (t.to(dt) for t in (x, p, z, go))
        sides[dt] = identities(dist2plane_matmul_ref, a, b, c, lambda u, v, w, g=g: dist2plane_matmul_bwd(u, v, w, g))

    def dev_bwd(u, v, w):
        leaves = [t.clone().requires_grad_(True) for t in (u, v, w)]
        return torch.autograd.grad(gm.dist2plane_matmul(*leaves, k=-1.0), leaves, go.float().cuda())

    dev = identities(lambda u, v, w: gm.dist2plane_matmul(u, v, w, k=-1.0), x.float().cuda(), p.float().cuda(), z.float().cuda(), dev_bwd)
    failures = []
    for (name, l64, r64), (_, l32, r32), (_, lg, rg) in zip(sides[F64], sides[F32], dev):
        allow = 0.0
        for s64, s32 in ((l64, l32), (r64, r32)):
            scale = max(1.0, float(s64.abs().max()))
            allow += (C * float((s32.double() - s64).abs().max()) / scale + F) * scale
        diff = float((lg.double() - rg.double()).abs().max())
        print(f"\ndist2plane_matmul {shape} {name}: |left - right| / allowance {diff / allow:.3f}")
        if not diff <= allow:
            failures.append(f"{shape} {name}: {diff:.3e} > {allow:.3e}")
    assert not failures, "\n".join(failures)


# ================================================================================================ the same bits
def test_operands_at_storage_offset_1_give_the_same_bits():
    x, pp, zz, go = _data(2, 65, 129, 100)
    _equal(_run(x, pp, zz, go), _run(x, pp, zz, go, unaligned=True), "storage offset 1")


def test_a_transposed_view_and_materialised_planes_give_the_same_bits():
    x, pp, zz, go = _data(2, 65, 129, 100)
    view = _run(x, pp, zz, go)
    xd = x.cuda().requires_grad_(True)
    pm, zm = (t.cuda().transpose(-1, -2).contiguous().requires_grad_(True) for t in (pp, zz))      # (batch, D, M) in memory
    out = _gmath().dist2plane_matmul(xd, pm, zm, k=-1.0)
    out.backward(go.cuda())
    _equal([out.detach(), xd.grad, pm.grad.transpose(-1, -2).contiguous(), zm.grad.transpose(-1, -2).contiguous()], view, "materialised planes")


def test_each_null_gradient_combination_has_the_bits_of_the_full_run():
    c = _C()
    for batch, N, M, D in ((2, 17, 33, 20), (1, 20, 20, 129)):
        x, pp, zz, go = (t.cuda() for t in _data(batch, N, M, D))
        full = None
        for sel in (7, 6, 5, 4, 3, 2, 1, 0):
            outs = [torch.full(tuple(t.shape), NAN, device="cuda") if sel >> i & 1 else None for i, t in enumerate((x, pp, zz))]
            c.check(c.lib.hypad_dist2plane_matmul_bwd(c.ptr(x), c.ptr(pp), c.ptr(zz), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), c.ptr(outs[2]), batch, N,
                                                      M, D, c.stream()), f"bwd {sel:03b}")
            full = full or outs
            _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"bwd {sel:03b}")
        assert all(bool(torch.isfinite(t).all()) for t in full)
    # and through autograd: a gradient that is not needed is not asked for
    x, pp, zz, go = _data(2, 17, 33, 20)
    want = _run(x, pp, zz, go)
    for i in range(3):
        leaves = [t.cuda().requires_grad_(k == i) for k, t in enumerate((x, pp, zz))]
        out = _gmath().dist2plane_matmul(leaves[0], leaves[1].transpose(-1, -2), leaves[2].transpose(-1, -2), k=-1.0)
        out.backward(go.cuda())
        assert torch.equal(leaves[i].grad, want[1 + i]) and all(leaves[k].grad is None for k in range(3) if k != i)


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    L = c.lib
    cks = []
    for batch, N, M, D in ((2, 17, 33, 20), (1, 65, 63, 129)):
        x, pp, zz, go = _data(batch, N, M, D)
        res = _refs(None, x, pp, zz, go)
        xd, pd, zd, god = x.cuda(), pp.cuda(), zz.cuda(), go.cuda()
        bufs = [_guarded(s, o) for s, o in (((batch, N, M), 3), ((batch, N, D), 1), ((batch, M, D), 2), ((batch, M, D), 5))]
        (_, out), (_, gx), (_, gp), (_, gz) = bufs
        c.check(L.hypad_dist2plane_matmul_fwd(c.ptr(xd), c.ptr(pd), c.ptr(zd), c.ptr(out), batch, N, M, D, c.stream()))
        c.check(L.hypad_dist2plane_matmul_bwd(c.ptr(xd), c.ptr(pd), c.ptr(zd), c.ptr(god), c.ptr(gx), c.ptr(gp), c.ptr(gz), batch, N, M, D, c.stream()))
        torch.cuda.synchronize()
        for (buf, v), off in zip(bufs, (3, 1, 2, 5)):
            assert _guards_intact(buf, off)
        ck = Ck(f"guarded {(batch, N, M, D)}")
        _check(ck, res, (out, gx, gp, gz))
        cks.append(ck)
    _finish(cks)


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    batch, N, M = 2, 4, 6
    for D in (257, 8):
        x, pp, zz, go = (torch.zeros(s, device="cuda") for s in ((batch, N, D), (batch, M, D), (batch, M, D), (batch, N, M)))
        out, gx, gp, gz = (torch.full(s, SENTINEL, device="cuda") for s in ((batch, N, M), (batch, N, D), (batch, M, D), (batch, M, D)))
        fwd = lambda a=x, p=pp, z=zz, o=out, b=batch, n=N, m=M, d=D: L.hypad_dist2plane_matmul_fwd(c.ptr(a), c.ptr(p), c.ptr(z), c.ptr(o), b, n, m, d,
                                                                                                  c.stream())
        bwd = lambda a=x, p=pp, z=zz, g=go, b=batch, n=N, m=M, d=D: L.hypad_dist2plane_matmul_bwd(c.ptr(a), c.ptr(p), c.ptr(z), c.ptr(g), c.ptr(gx),
                                                                                                  c.ptr(gp), c.ptr(gz), b, n, m, d, c.stream())
        if D == 257:
            assert fwd() == bwd() == HYPAD_EUNSUPPORTED
        else:
            assert fwd(a=None) == fwd(p=None) == fwd(z=None) == fwd(o=None) == bwd(a=None) == bwd(p=None) == bwd(z=None) == bwd(g=None) == HYPAD_EINVAL
            assert fwd(b=-1) == fwd(n=-1) == fwd(m=-2) == fwd(d=0) == fwd(d=-3) == bwd(b=-1) == bwd(n=-4) == bwd(m=-1) == bwd(d=0) == HYPAD_EINVAL
            assert fwd(b=2 ** 20, n=2 ** 6, m=2 ** 5) == bwd(b=1, n=2 ** 16, m=2 ** 15) == HYPAD_EUNSUPPORTED      # 2^31 elements
        torch.cuda.synchronize()
        for t in (out, gx, gp, gz):
            assert bool((t == SENTINEL).all())              # nothing ran
    assert fwd() == 0 and bwd() == 0
    with pytest.raises(NotImplementedError, match="supported"):
        _gmath().dist2plane_matmul(torch.zeros(2, 4, 257, device="cuda"), torch.zeros(2, 257, 3, device="cuda"), torch.zeros(2, 257, 3, device="cuda"),
                                   k=-1.0)


def test_no_rows_no_planes_and_no_batch_leave_zero_gradients():
    c = _C()
    L = c.lib
    x6, e = torch.zeros(2, 6, 8, device="cuda"), None
    nan = lambda *s: torch.full(s, NAN, device="cuda")
    gp, gz = nan(2, 6, 8), nan(2, 6, 8)                     # N = 0: the planes (2, 6, 8) get zeros
    assert L.hypad_dist2plane_matmul_fwd(e, c.ptr(x6), c.ptr(x6), e, 2, 0, 6, 8, c.stream()) == 0
    assert L.hypad_dist2plane_matmul_bwd(e, c.ptr(x6), c.ptr(x6), e, e, c.ptr(gp), c.ptr(gz), 2, 0, 6, 8, c.stream()) == 0
    assert bool((gp == 0).all()) and bool((gz == 0).all())
    gx = nan(2, 6, 8)                                       # M = 0: x (2, 6, 8) gets zeros
    assert L.hypad_dist2plane_matmul_bwd(c.ptr(x6), e, e, e, c.ptr(gx), e, e, 2, 6, 0, 8, c.stream()) == 0
    assert bool((gx == 0).all())
    assert L.hypad_dist2plane_matmul_fwd(e, e, e, e, 0, 5, 6, 8, c.stream()) == 0 and L.hypad_dist2plane_matmul_bwd(e, e, e, e, e, e, e, 0, 5, 6, 8, c.stream()) == 0
    gm = _gmath()
    for shape_x, shape_p in (((2, 0, 8), (2, 6, 8)), ((2, 5, 8), (2, 0, 8)), ((0, 5, 8), (0, 6, 8))):
        xd = torch.zeros(shape_x, device="cuda", requires_grad=True)
        pd, zd = (torch.zeros(shape_p, device="cuda", requires_grad=True) for _ in range(2))
        out = gm.dist2plane_matmul(xd, pd.transpose(-1, -2), zd.transpose(-1, -2), k=-1.0)
        assert out.shape == (shape_x[0], shape_x[1], shape_p[1])
        out.sum().backward()
        for t in (xd, pd, zd):
            assert t.grad.shape == t.shape and bool((t.grad == 0).all())


# ================================================================================================ side stream, captured graph
def _fwd_bwd(a, b, c_, go):
    out = _gmath().dist2plane_matmul(a, b.transpose(-1, -2), c_.transpose(-1, -2), k=-1.0)
    return (out,) + torch.autograd.grad(out, [a, b, c_], go)


def _leaves(host):
    a, b, c_, go = (t.cuda() for t in host)
    return a.requires_grad_(True), b.requires_grad_(True), c_.requires_grad_(True), go


def test_on_a_side_stream():
    host = _data(2, 65, 129, 100)
    want = [t.clone() for t in _fwd_bwd(*_leaves(host))]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _fwd_bwd(*_leaves(host))                      # placed and filled on the side stream: a launch on stream 0 would race them
    side.synchronize()
    _equal(got, want, "on a side stream")


def test_captured_and_replayed_with_changed_inputs():
    host = _data(2, 65, 129, 100)
    g = torch.Generator().manual_seed(11)
    second = (host[0].flip(0).contiguous(), (host[1] * 0.5).contiguous(), host[2].flip(1).contiguous(), torch.randn(host[3].shape, generator=g))
    wants = [[t.clone() for t in _fwd_bwd(*_leaves(h))] for h in (host, second)]
    assert not torch.equal(wants[0][0], wants[1][0])
    static = list(_leaves(host))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _fwd_bwd(*static)                                   # the eager warm-up, on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = _fwd_bwd(*static)
    for i in (1, 0):                                        # replayed twice, each time with other inputs
        with torch.no_grad():
            for s, h in zip(static, (host, second)[i]):
                s.copy_(h.cuda())
        graph.replay()
        torch.cuda.synchronize()
        _equal([t.detach() for t in outs], wants[i], f"replay with data set {i}")


# ================================================================================================ the block
def test_attention_block_with_per_batch_planes():
    """hyperbolic_attention -> dist2plane_matmul against planes of each batch element's own -> cross-entropy: every gradient against the
    same chain in torch (attention_ref, dist2plane_matmul_ref)."""
    from attention_ref import hyperbolic_attention_ref
    batch, N, M, D, classes, beta = 2, 9, 11, 20, 5, 1.7
    g = torch.Generator().manual_seed(21252159)
    ball = lambda rows: _ball_rows(g, batch * rows, D, edge=False, radius=0.8, zero_row=False).reshape(batch, rows, D)
    q, keys, values, points = ball(N), ball(M), ball(M), ball(classes)
    normals, target = torch.randn(batch, classes, D, generator=g), torch.randint(0, classes, (batch * N,), generator=g)
    names = ("q", "keys", "values", "points", "normals")
    res = {}
    for dt in (F64, F32):
        t = {n: _leaf(v, dt) for n, v in zip(names, (q, keys, values, points, normals))}
        mid = hyperbolic_attention_ref(t["q"], t["keys"], t["values"], beta)
        logits = dist2plane_matmul_ref(mid, t["points"].transpose(-1, -2), t["normals"].transpose(-1, -2))
        loss = torch.nn.functional.cross_entropy(logits.reshape(batch * N, classes), target)
        gs = torch.autograd.grad(loss, [t[n] for n in names])
        res[dt] = dict(mid=mid.detach(), logits=logits.detach(), loss=loss.detach(), **{"g_" + n: v for n, v in zip(names, gs)})
    gm = _gmath()
    d = {n: v.cuda().requires_grad_(True) for n, v in zip(names, (q, keys, values, points, normals))}
    mid = gm.hyperbolic_attention(d["q"], d["keys"], d["values"], -1.0, beta=beta)
    logits = gm.dist2plane_matmul(mid, d["points"].transpose(-1, -2), d["normals"].transpose(-1, -2), k=-1.0)
    loss = torch.nn.functional.cross_entropy(logits.reshape(batch * N, classes), target.cuda())
    loss.backward()
    ck = Ck("attention block (2, 9, 11, 20)")
    for name, t in [("mid", mid.detach()), ("logits", logits.detach()), ("loss", loss.detach())] + [("g_" + n, d[n].grad) for n in names]:
        assert bool(torch.isfinite(t).all()), name
        ck.cmp(name, t.cpu(), res[F64][name], res[F32][name])
    _report(ck.case, [ck])
    _finish([ck])
