"""The geodesic distances dist_matmul, dist and dist0 on the GPU (hypad_dist_matmul_*, hypad_dist_*, hypad_dist0_*; hyperspace/gmath
runs them) against the plain-torch restatement of tests/dist_ref.py -- which tests/test_dist_host.py pins to the reference's own
outputs -- run in fp64 and fp32 on the CPU, under the project's rule ``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1).
No tolerance of its own, with one exception that is a bound and not a tolerance: the diagonal of a self-distance matrix (below).

The data.  Points: ``_ball_rows`` (radius <= 0.95, the last row all zero, no rim row); grad_out ~ N(0, 1).  A point on the 1 - 1e-3 norm
moves err32 of every tensor it touches, so it gets a test of its own per shape and does not set err32 for the others.

Tile and chunk sizes of the kernels (csrc/dist.hip), each with a shape at, one below and one above it in ``PAIR_EDGES``:
    forward: 64 x 64 tiles of out, D in chunks of 128     N (1,63..65,20,20), M (1,20,63..65,20), D (1,20,20,127..129), (1,16,260,256)
    backward: 64 own rows, the other operand in chunks of 64 points, accumulator classes D <= 64 / 128 / 256
                                                          the same shapes: grad_x walks M and owns N, grad_y walks N and owns M;
                                                          D (1,20,20,63), (1,64,100,64), (1,20,20,65), (1,20,20,127..129), (1,16,260,256)
    65 chunks: (1,17,4099,20) for grad_x, (1,4099,17,20) for grad_y
The row forms have no tile: a wave per row, 64 lanes x 4 elements (D = 1, 63, 100, 256 cover one to four elements a lane).

The diagonal of dist_matmul(x, x^T).  num = x2 - 2 xy + x2 is a difference of equal quantities there, each form rounds it its own way
(the reference's fp32 diagonal reads up to 1.6e-3), so it is not compared with the restatement.  The kernel's x2 is an fp64 sum of the
fp32 values and its xy an fp32 dot product of length D, so |num| <= (D + 2) 2^-23 |x|^2 and
    0 < out_ii <= 2 artanh(sqrt(max(1e-15, (D + 2) 2^-23 |x_i|^2)) / (1 - |x_i|^2)),
the right side rounded up to fp32, the format out is stored in (an all-zero row meets it with equality).
"""
import numpy as np
import pytest
import torch

from dist_ref import dist0_ref, dist_matmul_ref, dist_ref
from sweep_common import NAN, SENTINEL, Ck, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                 # include/hypad.h
PAIR_SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (3, 17, 33, 20), (1, 64, 100, 64), (2, 65, 129, 100), (1, 16, 260, 256)]   # (batch, N, M, D)
PAIR_EDGES = [(1, 63, 20, 20), (1, 65, 20, 20), (1, 20, 63, 20), (1, 20, 64, 20), (1, 20, 65, 20), (1, 20, 20, 63), (1, 20, 20, 65),
              (1, 20, 20, 127), (1, 20, 20, 128), (1, 20, 20, 129)]
PAIR_LONG = [(1, 17, 4099, 20), (1, 4099, 17, 20)]
ROW_SHAPES = [(39, 100), (17, 256), (1, 1), (5, 63)]


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
    print(f"\ngeodesic distance {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _equal(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def _rim(x2d, g):
    """One row of a (rows, D) matrix moved to the 1 - 1e-3 norm (a zero row gets a direction first)."""
    i = 1 if x2d.shape[0] >= 3 else 0
    v = x2d[i].double()
    if float(v.norm()) == 0:
        v = torch.randn(v.shape, generator=g, dtype=F64)
    x2d[i] = (v * ((1 - 1e-3) / float(v.norm()))).float()
    return x2d


# ================================================================================================ pair form
def _pair_data(batch, N, M, D, rim=False, radius=0.95, seed=0):
    """x (batch, N, D), the points of y (batch, M, D), grad_out (batch, N, M)."""
    g = torch.Generator().manual_seed(1000003 * batch + 10007 * N + 101 * M + D + seed)
    x = _ball_rows(g, batch * N, D, edge=False, radius=radius)
    yp = _ball_rows(g, batch * M, D, edge=False, radius=radius)
    if rim:
        x = _rim(x, g)
    return x.reshape(batch, N, D), yp.reshape(batch, M, D), torch.randn(batch, N, M, generator=g)


_REFS = {}


def _pair_refs(key, x, yp, go):
    """out, grad_x, grad of the points of y, of the restatement in fp64 and fp32 (computed once per key)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        xx, yy = _leaf(x, dt), _leaf(yp, dt)
        o = dist_matmul_ref(xx, yy.transpose(-1, -2))
        gx, gy = torch.autograd.grad(o, [xx, yy], go.to(dt))
        res[dt] = dict(out=o.detach(), gx=gx, gy=gy)
    if key is not None:
        _REFS[key] = res
    return res


def _pair_run(x, yp, go, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, yd = mk(x).requires_grad_(True), mk(yp).requires_grad_(True)
    out = _gmath().dist_matmul(xd, yd.transpose(-1, -2), -1.0)
    out.backward(go.cuda())
    return out.detach(), xd.grad, yd.grad


def _pair_check(ck, res, out, gx, gy):
    for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_y", gy, "gy")):
        assert bool(torch.isfinite(t).all()), (ck.case, name)
        ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])


def _pair_case(shape, tag, rim=False):
    x, yp, go = _pair_data(*shape, rim=rim)
    ck = Ck(f"dist_matmul {shape} {tag}")
    _pair_check(ck, _pair_refs((shape, rim), x, yp, go), *_pair_run(x, yp, go))
    return ck


@pytest.mark.parametrize("shape", PAIR_SHAPES + PAIR_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_pair_forward_and_backward(shape):
    ck = _pair_case(shape, "")
    _report(ck.case, [ck])
    _finish([ck])


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pair_rim_point(shape):
    ck = _pair_case(shape, "rim point", rim=True)
    _report(ck.case, [ck])
    _finish([ck])


@pytest.mark.parametrize("shape", PAIR_LONG, ids=lambda s: "x".join(map(str, s)))
def test_pair_walk_of_65_chunks_twice_the_same_bits(shape):
    x, yp, go = _pair_data(*shape)
    got = []
    for _ in range(2):
        got.append(_pair_run(x, yp, go))
        torch.full((4099 * 20 * 7,), NAN, device="cuda")    # (another history of the allocator's blocks between the runs)
    _equal(got[0], got[1], f"dist_matmul {shape}")
    ck = Ck(f"dist_matmul {shape}: 65 chunks")
    _pair_check(ck, _pair_refs(None, x, yp, go), *got[0])
    _report(ck.case, [ck])
    _finish([ck])


def test_pair_batch_dimensions_and_an_operand_without_them():
    """Leading batch dimensions (2, 3) on both operands; then x without them and y without them: the operand is expanded on the host and
    autograd sums its gradient over the batch."""
    g = torch.Generator().manual_seed(29)
    x = _ball_rows(g, 6 * 4, 5, edge=False).reshape(2, 3, 4, 5)
    yp = _ball_rows(g, 6 * 7, 5, edge=False).reshape(2, 3, 7, 5)
    go = torch.randn(2, 3, 4, 7, generator=g)
    cks = []
    for tag, x_, y_ in (("both", x, yp), ("x shared", x[0, 0], yp), ("y shared", x, yp[0, 0])):
        res = _pair_refs(None, x_, y_, go)
        out, gx, gy = _pair_run(x_, y_, go)
        assert out.shape == (2, 3, 4, 7) and gx.shape == x_.shape and gy.shape == y_.shape
        ck = Ck("dist_matmul batch dims, " + tag)
        _pair_check(ck, res, out, gx, gy)
        cks.append(ck)
    _report("batch dims", cks)
    _finish(cks)


@pytest.mark.parametrize("n,D", [(64, 64), (20, 3)])
def test_self_distance(n, D):
    g = torch.Generator().manual_seed(100 * n + D)
    x = _ball_rows(g, n, D, edge=False, radius=0.8).reshape(1, n, D)
    off = ~np.eye(n, dtype=bool)[None]
    go = torch.randn(1, n, n, generator=g) * torch.from_numpy(off).float()            # a zero diagonal
    res = {}
    for dt in (F64, F32):
        xx = _leaf(x, dt)
        o = dist_matmul_ref(xx, xx.transpose(-1, -2))
        res[dt] = dict(out=o.detach(), gx=torch.autograd.grad(o, xx, go.to(dt))[0])
    xd = x.cuda().requires_grad_(True)
    out = _gmath().dist_matmul(xd, xd.transpose(-1, -2), -1.0)
    (gx,) = torch.autograd.grad(out, xd, go.cuda(), retain_graph=True)
    ck = Ck(f"self-distance ({n}, {D})")
    ck.cmp("out off the diagonal", out.detach().cpu(), res[F64]["out"], res[F32]["out"], mask=off)
    ck.cmp("grad_x under a zero-diagonal grad_out", gx.cpu(), res[F64]["gx"], res[F32]["gx"])
    x2 = x[0].double().pow(2).sum(-1).numpy()
    bound = 2 * np.arctanh(np.sqrt(np.maximum(1e-15, (D + 2) * 2.0 ** -23 * x2)) / (1 - x2))
    bound32 = np.nextafter(bound.astype(np.float32), np.float32(np.inf))
    diag = out.detach().cpu()[0].diagonal().numpy()
    print(f"\nself-distance ({n}, {D}): worst diagonal / bound {float((diag / bound).max()):.3f}, over the rows that are not zero "
          f"{float((diag / bound)[x2 > 0].max()):.3f}")
    assert (diag > 0).all() and (diag <= bound32).all(), (diag / bound).max()
    (gfull,) = torch.autograd.grad(out, xd, torch.randn(1, n, n, generator=g).cuda())
    assert bool(torch.isfinite(gfull).all())
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ row forms
def _row_data(rows, D, rim=False):
    """x and y (rows, D); from five rows on: y row 0 all zero, row 2 the same point in both, row 3 zero in both, the last row of x all
    zero; rim: x row 1 (or 0) on the 1 - 1e-3 norm."""
    g = torch.Generator().manual_seed(1009 * rows + D)
    x = _ball_rows(g, rows, D, edge=False)
    y = _ball_rows(g, rows, D, edge=False, zero_row=False)
    if rim:
        x = _rim(x, g)
    if rows >= 5:
        y[0] = 0.0
        y[2] = x[2]
        x[3] = 0.0
        y[3] = 0.0
    return x, y, torch.randn(rows, generator=g)


def _row_refs(x, y, go):
    res = {}
    for dt in (F64, F32):
        xx, yy = _leaf(x, dt), _leaf(y, dt)
        o = dist_ref(xx, yy)
        gx, gy = torch.autograd.grad(o, [xx, yy], go.to(dt))
        x0 = _leaf(x, dt)
        o0 = dist0_ref(x0)
        res[dt] = dict(out=o.detach(), gx=gx, gy=gy, out0=o0.detach(), gx0=torch.autograd.grad(o0, x0, go.to(dt))[0])
    return res


def _row_run(x, y, go, unaligned=False, keepdim=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    gm = _gmath()
    xd, yd, x0 = mk(x).requires_grad_(True), mk(y).requires_grad_(True), mk(x).requires_grad_(True)
    god = go.cuda().reshape(-1, 1) if keepdim else go.cuda()
    out = gm.dist(xd, yd, k=-1.0, keepdim=keepdim)
    out.backward(god)
    out0 = gm.dist0(x0, k=-1.0, keepdim=keepdim)
    out0.backward(god)
    return out.detach(), xd.grad, yd.grad, out0.detach(), x0.grad


@pytest.mark.parametrize("rim", [False, True], ids=["inside", "rim"])
@pytest.mark.parametrize("rows,D", ROW_SHAPES)
def test_row_forms_forward_and_backward(rows, D, rim):
    """The equal pair (row 2) is left out of the comparison of dist with the restatement -- (-x) (+) x is zero there only up to the
    rounding of two coefficients, and the gradient through a norm of 1e-16 is noise in any precision -- and held to what the distance of
    a point from itself is: 0, with gradient 0, exactly.  The pair of zero rows (row 3) is compared like every other row."""
    x, y, go = _row_data(rows, D, rim=rim)
    res = _row_refs(x, y, go)
    out, gx, gy, out0, gx0 = _row_run(x, y, go)
    assert out.shape == out0.shape == (rows,)
    live = np.ones(rows, dtype=bool)
    if rows >= 5:
        live[2] = False
        assert float(out[2]) == 0.0 and bool((gx[2] == 0).all()) and bool((gy[2] == 0).all())
        assert float(out[3]) == 0.0 and bool((gx[3] == 0).all()) and bool((gy[3] == 0).all())
        assert float(out0[3]) == 0.0 and bool((gx0[3] == 0).all()) and bool((gx0[-1] == 0).all())
    live2 = live[:, None] & np.ones((rows, D), dtype=bool)
    ck = Ck(f"row forms ({rows}, {D}) rim={rim}")
    r64, r32 = res[F64], res[F32]
    for t in (out, gx, gy, out0, gx0):
        assert bool(torch.isfinite(t).all())
    ck.cmp("dist out", out.cpu(), r64["out"], r32["out"], mask=live)
    ck.cmp("dist grad_x", gx.cpu(), r64["gx"], r32["gx"], mask=live2)
    ck.cmp("dist grad_y", gy.cpu(), r64["gy"], r32["gy"], mask=live2)
    ck.cmp("dist0 out", out0.cpu(), r64["out0"], r32["out0"])
    ck.cmp("dist0 grad_x", gx0.cpu(), r64["gx0"], r32["gx0"])
    kd = _row_run(x, y, go, keepdim=True)
    assert kd[0].shape == kd[3].shape == (rows, 1)
    _equal([kd[0].reshape(-1), kd[1], kd[2], kd[3].reshape(-1), kd[4]], [out, gx, gy, out0, gx0], "keepdim")
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ the reference's recorded cases
def test_recorded_cases_through_the_public_functions():
    from test_dist_host import ROW_EQUAL, ROW_ZERO_BOTH, ROW_ZERO_X, load_fixture
    gm = _gmath()
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    x, y, go = fx["dm_x"], fx["dm_y"], fx["dm_grad_output"]
    res = _pair_refs(None, x, y.transpose(-1, -2).contiguous(), go)
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)       # y as recorded: (batch, D, M), materialised
    out = gm.dist_matmul(xd, yd, -1.0)
    out.backward(go.cuda())
    ck = Ck("recorded dm")
    _pair_check(ck, res, out.detach(), xd.grad, yd.grad.transpose(-1, -2))
    assert abs(float(out.detach()[0, 2, 4]) - 2 * np.arctanh(np.sqrt(1e-15))) <= 1e-6 * 2 * np.arctanh(np.sqrt(1e-15))      # the zero / zero pair
    rx, ry, rgo = fx["row_x"], fx["row_y"], fx["row_grad_output"]
    rres = _row_refs(rx, ry, rgo)
    o, gx, gy, o0, gx0 = _row_run(rx, ry, rgo)
    ck2 = Ck("recorded rows")
    for name, t, k in (("dist out", o, "out"), ("dist grad_x", gx, "gx"), ("dist grad_y", gy, "gy"), ("dist0 out", o0, "out0"), ("dist0 grad_x", gx0, "gx0")):
        ck2.cmp(name, t.cpu(), rres[F64][k], rres[F32][k])
    for row in (ROW_EQUAL, ROW_ZERO_BOTH):
        assert float(o[row]) == 0.0 and bool((gx[row] == 0).all()) and bool((gy[row] == 0).all())
    assert float(o0[ROW_ZERO_X]) == 0.0 and bool((gx0[ROW_ZERO_X] == 0).all())
    _report("recorded cases", [ck, ck2])
    _finish([ck, ck2])


# ================================================================================================ the same bits
def test_operands_at_storage_offset_1_give_the_same_bits():
    x, yp, go = _pair_data(2, 65, 129, 100)
    _equal(_pair_run(x, yp, go), _pair_run(x, yp, go, unaligned=True), "dist_matmul")
    x, y, go = _row_data(39, 100)
    _equal(_row_run(x, y, go), _row_run(x, y, go, unaligned=True), "row forms")


def test_a_transposed_view_and_a_materialised_y_give_the_same_bits():
    x, yp, go = _pair_data(2, 65, 129, 100)
    view = _pair_run(x, yp, go)
    xd = x.cuda().requires_grad_(True)
    ym = yp.cuda().transpose(-1, -2).contiguous().requires_grad_(True)           # (batch, D, M) in memory
    out = _gmath().dist_matmul(xd, ym, -1.0)
    out.backward(go.cuda())
    _equal([out.detach(), xd.grad, ym.grad.transpose(-1, -2).contiguous()], view, "materialised y")


def test_each_null_gradient_combination_has_the_bits_of_the_full_run():
    c = _C()
    batch, N, M, D = 2, 17, 33, 20
    x, yp, go = (t.cuda() for t in _pair_data(batch, N, M, D))
    full = None
    for sel in (3, 2, 1, 0):
        outs = [torch.full(tuple(t.shape), NAN, device="cuda") if sel >> i & 1 else None for i, t in enumerate((x, yp))]
        c.check(c.lib.hypad_dist_matmul_bwd(c.ptr(x), c.ptr(yp), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), batch, N, M, D, c.stream()), f"bwd {sel:02b}")
        full = full or outs
        _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"dist_matmul {sel:02b}")
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all())
    x, y, go = (t.cuda() for t in _row_data(39, 100))
    full = None
    for sel in (3, 2, 1, 0):
        outs = [torch.full((39, 100), NAN, device="cuda") if sel >> i & 1 else None for i in range(2)]
        c.check(c.lib.hypad_dist_bwd(c.ptr(x), c.ptr(y), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), 39, 100, c.stream()), f"dist_bwd {sel:02b}")
        full = full or outs
        _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"dist {sel:02b}")
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all())


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    L = c.lib
    cks = []
    for batch, N, M, D in ((2, 17, 33, 20), (1, 65, 63, 129)):
        x, yp, go = _pair_data(batch, N, M, D)
        res = _pair_refs(None, x, yp, go)
        xd, yd, god = x.cuda(), yp.cuda(), go.cuda()
        bufs = [_guarded(s, o) for s, o in (((batch, N, M), 3), ((batch, N, D), 1), ((batch, M, D), 2))]
        (_, out), (_, gx), (_, gy) = bufs
        c.check(L.hypad_dist_matmul_fwd(c.ptr(xd), c.ptr(yd), c.ptr(out), batch, N, M, D, c.stream()))
        c.check(L.hypad_dist_matmul_bwd(c.ptr(xd), c.ptr(yd), c.ptr(god), c.ptr(gx), c.ptr(gy), batch, N, M, D, c.stream()))
        torch.cuda.synchronize()
        for (buf, v), off in zip(bufs, (3, 1, 2)):
            assert _guards_intact(buf, off)
        ck = Ck(f"guarded dist_matmul {(batch, N, M, D)}")
        _pair_check(ck, res, out, gx, gy)
        cks.append(ck)
    rows, D = 17, 256
    x, y, go = _row_data(rows, D)
    res = _row_refs(x, y, go)
    xd, yd, god = x.cuda(), y.cuda(), go.cuda()
    bufs = [_guarded(s, o) for s, o in (((rows,), 3), ((rows, D), 1), ((rows, D), 2), ((rows,), 5), ((rows, D), 7))]
    (_, out), (_, gx), (_, gy), (_, out0), (_, gx0) = bufs
    c.check(L.hypad_dist_fwd(c.ptr(xd), c.ptr(yd), c.ptr(out), rows, D, c.stream()))
    c.check(L.hypad_dist_bwd(c.ptr(xd), c.ptr(yd), c.ptr(god), c.ptr(gx), c.ptr(gy), rows, D, c.stream()))
    c.check(L.hypad_dist0_fwd(c.ptr(xd), c.ptr(out0), rows, D, c.stream()))
    c.check(L.hypad_dist0_bwd(c.ptr(xd), c.ptr(god), c.ptr(gx0), rows, D, c.stream()))
    torch.cuda.synchronize()
    for (buf, v), off in zip(bufs, (3, 1, 2, 5, 7)):
        assert _guards_intact(buf, off)
    live = np.ones(rows, dtype=bool)
    live[2] = False
    live2 = live[:, None] & np.ones((rows, D), dtype=bool)
    ck = Ck("guarded row forms (17, 256)")
    ck.cmp("dist out", out.cpu(), res[F64]["out"], res[F32]["out"], mask=live)
    ck.cmp("dist grad_x", gx.cpu(), res[F64]["gx"], res[F32]["gx"], mask=live2)
    ck.cmp("dist grad_y", gy.cpu(), res[F64]["gy"], res[F32]["gy"], mask=live2)
    ck.cmp("dist0 out", out0.cpu(), res[F64]["out0"], res[F32]["out0"])
    ck.cmp("dist0 grad_x", gx0.cpu(), res[F64]["gx0"], res[F32]["gx0"])
    _finish(cks + [ck])


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    batch, N, M = 2, 4, 6
    for D in (257, 8):
        x, yp, go = (torch.zeros(s, device="cuda") for s in ((batch, N, D), (batch, M, D), (batch, N, M)))
        out, gx, gy, rout = (torch.full(s, SENTINEL, device="cuda") for s in ((batch, N, M), (batch, N, D), (batch, M, D), (batch * N,)))
        fwd = lambda a=x, b_=yp, o=out, b=batch, n=N, m=M, d=D: L.hypad_dist_matmul_fwd(c.ptr(a), c.ptr(b_), c.ptr(o), b, n, m, d, c.stream())
        bwd = lambda a=x, b_=yp, g=go, b=batch, n=N, m=M, d=D: L.hypad_dist_matmul_bwd(c.ptr(a), c.ptr(b_), c.ptr(g), c.ptr(gx), c.ptr(gy), b, n, m, d,
                                                                                      c.stream())
        # the row forms over the batch * N rows of x, with gx's storage as the second operand's gradient too
        rfwd = lambda a=x, b_=x, o=rout, r=batch * N, d=D: L.hypad_dist_fwd(c.ptr(a), c.ptr(b_), c.ptr(o), r, d, c.stream())
        rbwd = lambda a=x, b_=x, g=go, r=batch * N, d=D: L.hypad_dist_bwd(c.ptr(a), c.ptr(b_), c.ptr(g), c.ptr(gx), None, r, d, c.stream())
        zfwd = lambda a=x, o=rout, r=batch * N, d=D: L.hypad_dist0_fwd(c.ptr(a), c.ptr(o), r, d, c.stream())
        zbwd = lambda a=x, g=go, o=gx, r=batch * N, d=D: L.hypad_dist0_bwd(c.ptr(a), c.ptr(g), c.ptr(o), r, d, c.stream())
        if D == 257:
            for call in (fwd, bwd, rfwd, rbwd, zfwd, zbwd):
                assert call() == HYPAD_EUNSUPPORTED
        else:
            assert fwd(a=None) == fwd(b_=None) == fwd(o=None) == bwd(a=None) == bwd(b_=None) == bwd(g=None) == HYPAD_EINVAL
            assert fwd(b=-1) == fwd(n=-1) == fwd(m=-2) == fwd(d=0) == fwd(d=-3) == bwd(b=-1) == bwd(n=-4) == bwd(m=-1) == bwd(d=0) == HYPAD_EINVAL
            assert fwd(b=2 ** 20, n=2 ** 6, m=2 ** 5) == bwd(b=1, n=2 ** 16, m=2 ** 15) == HYPAD_EUNSUPPORTED      # 2^31 distances
            assert rfwd(a=None) == rfwd(b_=None) == rfwd(o=None) == rfwd(r=-1) == rfwd(d=0) == HYPAD_EINVAL
            assert rbwd(a=None) == rbwd(b_=None) == rbwd(g=None) == rbwd(r=-1) == rbwd(d=-1) == HYPAD_EINVAL
            assert zfwd(a=None) == zfwd(o=None) == zfwd(r=-1) == zfwd(d=0) == zbwd(a=None) == zbwd(g=None) == zbwd(o=None) == zbwd(r=-2) == HYPAD_EINVAL
        torch.cuda.synchronize()
        for t in (out, gx, gy, rout):
            assert bool((t == SENTINEL).all())              # nothing ran
    assert fwd() == 0 and bwd() == 0 and rfwd() == 0 and rbwd() == 0 and zfwd() == 0 and zbwd() == 0
    with pytest.raises(NotImplementedError, match="supported"):
        _gmath().dist_matmul(torch.zeros(2, 4, 257, device="cuda"), torch.zeros(2, 257, 3, device="cuda"), -1.0)


def test_no_pairs_and_no_rows_leave_zero_gradients():
    c = _C()
    L = c.lib
    x, yp = torch.zeros(2, 0, 8, device="cuda"), torch.zeros(2, 6, 8, device="cuda")
    gy = torch.full((2, 6, 8), NAN, device="cuda")
    assert L.hypad_dist_matmul_fwd(None, c.ptr(yp), None, 2, 0, 6, 8, c.stream()) == 0
    assert L.hypad_dist_matmul_bwd(None, c.ptr(yp), None, None, c.ptr(gy), 2, 0, 6, 8, c.stream()) == 0
    assert bool((gy == 0).all())
    gx = torch.full((2, 6, 8), NAN, device="cuda")          # and no points in y: x (2, 6, 8)
    assert L.hypad_dist_matmul_bwd(c.ptr(yp), None, None, c.ptr(gx), None, 2, 6, 0, 8, c.stream()) == 0
    assert bool((gx == 0).all())
    assert L.hypad_dist_fwd(None, None, None, 0, 8, c.stream()) == 0 and L.hypad_dist_bwd(None, None, None, None, None, 0, 8, c.stream()) == 0
    assert L.hypad_dist0_fwd(None, None, 0, 8, c.stream()) == 0 and L.hypad_dist0_bwd(None, None, None, 0, 8, c.stream()) == 0
    gm = _gmath()
    xd, yd = x.requires_grad_(True), yp.requires_grad_(True)
    out = gm.dist_matmul(xd, yd.transpose(-1, -2), -1.0)
    assert out.shape == (2, 0, 6)
    out.sum().backward()
    assert bool((yd.grad == 0).all()) and xd.grad.shape == (2, 0, 8)
    assert gm.dist(x.detach().reshape(0, 8), x.detach().reshape(0, 8), k=-1.0).shape == (0,) and gm.dist0(x.detach(), k=-1.0).shape == (2, 0)


# ================================================================================================ side stream, captured graph
def _stream_cases():
    x, yp, go = _pair_data(2, 65, 129, 100)
    rx, ry, rgo = _row_data(39, 100)
    gm = _gmath()
    return [("dist_matmul", (x, yp, go), lambda a, b: gm.dist_matmul(a, b.transpose(-1, -2), -1.0)),
            ("dist", (rx, ry, rgo), lambda a, b: gm.dist(a, b, k=-1.0) + gm.dist0(a, k=-1.0))]


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


# ================================================================================================ the block
def test_distance_attention_block():
    """softmax(-beta dist_matmul(q, keys^T)) -> weighted_midpoint_bmm(values, .) -> MobiusDist2Hyperplane -> cross-entropy: hyperbolic
    attention from the score to the loss, every gradient against the same chain in torch (dist_ref, midpoint_ref, dist2plane_ref)."""
    from dist2plane_ref import dist2plane_parts
    from hypad_amd.hyperspace import hyrnn_nets
    from midpoint_ref import weighted_midpoint_bmm_ref
    batch, N, M, D, C, beta = 2, 9, 11, 20, 5, 1.7
    g = torch.Generator().manual_seed(905947)
    q = _ball_rows(g, batch * N, D, edge=False, radius=0.8).reshape(batch, N, D)
    keys = _ball_rows(g, batch * M, D, edge=False, radius=0.8).reshape(batch, M, D)
    values = _ball_rows(g, batch * M, D, edge=False, radius=0.8).reshape(batch, M, D)
    point, tangent = _ball_rows(g, C, D, radius=0.8, edge=False, zero_row=False), torch.randn(C, D, generator=g)
    scale, target = 0.3 * torch.randn(C, generator=g), torch.randint(0, C, (batch * N,), generator=g)
    names = ("q", "keys", "values", "point", "tangent", "scale")
    res = {}
    for dt in (F64, F32):
        p = {n: _leaf(t, dt) for n, t in zip(names, (q, keys, values, point, tangent, scale))}
        score = dist_matmul_ref(p["q"], p["keys"].transpose(-1, -2))
        w = torch.softmax(-beta * score, dim=-1)
        mid = weighted_midpoint_bmm_ref(p["values"], w)
        logits, _ = dist2plane_parts(mid.reshape(batch * N, D), p["point"], p["tangent"], True, False, p["scale"])
        loss = torch.nn.functional.cross_entropy(logits, target)
        gs = torch.autograd.grad(loss, [p[n] for n in names])
        res[dt] = dict(score=score.detach(), mid=mid.detach(), logits=logits.detach(), loss=loss.detach(), **{"g_" + n: v for n, v in zip(names, gs)})
    head = hyrnn_nets.MobiusDist2Hyperplane(D, C)
    with torch.no_grad():
        head.point.copy_(point), head.tangent.copy_(tangent), head.scale.copy_(scale)
    head = head.cuda()
    d = {n: t.cuda().requires_grad_(True) for n, t in zip(names[:3], (q, keys, values))}
    gm = _gmath()
    score = gm.dist_matmul(d["q"], d["keys"].transpose(-1, -2), -1.0)
    w = torch.softmax(-beta * score, dim=-1)
    mid = gm.weighted_midpoint_bmm(d["values"], w, -1.0)
    logits = head(mid.reshape(batch * N, D))
    loss = torch.nn.functional.cross_entropy(logits, target.cuda())
    loss.backward()
    ck = Ck("distance attention block (2, 9, 11, 20)")
    r64, r32 = res[F64], res[F32]
    for name, t in (("score", score.detach()), ("mid", mid.detach()), ("logits", logits.detach()), ("loss", loss.detach()), ("g_q", d["q"].grad),
                    ("g_keys", d["keys"].grad), ("g_values", d["values"].grad), ("g_point", head.point.grad), ("g_tangent", head.tangent.grad),
                    ("g_scale", head.scale.grad)):
        assert bool(torch.isfinite(t).all()), name
        ck.cmp(name, t.cpu(), r64[name], r32[name])
    _report(ck.case, [ck])
    _finish([ck])
