"""dist2plane / MobiusDist2Hyperplane on the GPU (hypad_dist2plane_*; hyperspace/gmath.dist2plane and hyrnn_nets.MobiusDist2Hyperplane
run them) against the plain-torch restatement of tests/dist2plane_ref.py -- which tests/test_dist2plane_host.py pins to the reference's
own outputs -- run in fp64 and fp32 on the CPU, under the two rules of tests/test_gpu_dense_layers.py: per-row quantities (out, grad_x)
under ``Ck.cmp``, sums over rows (grad_p, grad_a, grad_scale) under ``Ck.red``.  No tolerance of its own.

The reductions.  The backward adds up, per plane n, the products of the per-element coefficients with x, p and a:
    grad_p[n] = sum_r C_px[r,n] x[r] + 2 C_p2[r,n] p[n] + C_pa[r,n] a[n]         grad_a[n] = sum_r C_xa[r,n] x[r] + C_pa[r,n] p[n] + C_an[r,n] a[n] / |a[n]|
    grad_scale[n] = sum_r grad_out[r,n] out[r,n]
``abs_terms`` is the fp64 sum of the absolute values of exactly these summands (the coefficients are the gradients of the six
(rows, N) nodes of ``dist2plane_parts``), and the summand allowance is the coefficients' own ``grad_allowance`` (fp32 restatement
against fp64) times the largest entry they multiply, as ``_reductions`` of tests/test_gpu_mobius_modes.py does for grad_weight.

The data.  x: rows within radius 0.9, the last one all zero, row 0 equal to the point of plane N // 2 (from three rows on); the planes'
points within radius 0.8, normals ~ N(0, 1) (not unit: ``scaled`` and the |a| gradient are live), log_scale ~ 0.3 N(0, 1).  A row on the
1 - 1e-3 norm is compared alone (``test_dist2plane_rim_row``).

The kink.  Row 0 lies ON plane N // 2.  The signed distance is smooth there; the unsigned one is |s| at s = 0, and the sign of that
pair's gradient is the sign of rounding noise -- in the reference's fp32 and fp64 runs as much as on the GPU.  The unsigned cases
therefore compare ``out`` whole and the gradients without what that pair feeds (row 0 of grad_x, plane N // 2 of grad_p and grad_a).
"""
import numpy as np
import pytest
import torch

import sweep_common as sc
from dist2plane_ref import dist2plane_parts, layer_ref
from sweep_common import NAN, SENTINEL, Ck, _at_offset, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EWORKSPACE, HYPAD_EUNSUPPORTED = -1, -2, -3          # include/hypad.h
SIGNED, SCALED = 1, 2                                                     # HYPAD_D2P_*
SHAPES = [(1, 1, 1), (3, 5, 7), (17, 33, 63), (64, 64, 64), (65, 100, 100), (39, 129, 65), (17, 256, 256), (130, 100, 200)]   # (rows, K, N)
ALL_FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # (signed, scaled)
PARTS = ("px", "xa", "x2", "p2", "pa", "an")


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\ndist2plane {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")


def _data(g, rows, K, N, rim=False):
    x = _ball_rows(g, rows, K, radius=0.9, edge=False).double()
    p = _ball_rows(g, N, K, radius=0.8, edge=False, zero_row=False)
    a = torch.randn(N, K, generator=g)
    if rows >= 3:
        x[0] = p[N // 2].double()
    if rim:
        i = 1 if rows >= 3 else 0
        x[i] *= (1 - 1e-3) / float(x[i].norm())
    return x.float(), p, a, 0.3 * torch.randn(N, generator=g), torch.randn(rows, N, generator=g)


_REFS = {}


def _refs(key, x, p, a, ls, go, signed, scaled):
    """fp64 and fp32 restatement of one case: out, the four gradients and the six coefficient matrices.  Computed once per key and
    shared (never modified)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        xx, pp, aa = _leaf(x, dt), _leaf(p, dt), _leaf(a, dt)
        ll = None if ls is None else _leaf(ls, dt)
        o, parts = dist2plane_parts(xx, pp, aa, signed, scaled, ll)
        gs = torch.autograd.grad(o, [xx, pp, aa] + ([] if ls is None else [ll]) + [parts[k] for k in PARTS], go.to(dt))
        nl = 3 if ls is None else 4
        res[dt] = dict(out=o.detach(), gx=gs[0], gp=gs[1], ga=gs[2], gs=None if ls is None else gs[3], go_out=(go.to(dt) * o.detach()),
                       **{k: c for k, c in zip(PARTS, gs[nl:])})
    if key is not None:
        _REFS[key] = res
    return res


def _reductions(ck, res, x, p, a, rows, gp, ga, gs, skip_plane=None):
    r64, r32 = res[F64], res[F32]
    x64, p64, a64 = x.double(), p.double(), a.double()
    an = a64.norm(dim=1, keepdim=True)
    al = {k: sc.grad_allowance(r64[k], r32[k]) for k in PARTS}
    col = lambda k: r64[k].abs().sum(0).unsqueeze(1)
    xm, pm, am = float(x64.abs().max()), float(p64.abs().max()), float(a64.abs().max())
    keep = [n for n in range(p.shape[0]) if n != skip_plane]
    if gp is not None:
        terms = r64["px"].abs().t() @ x64.abs() + 2 * col("p2") * p64.abs() + col("pa") * a64.abs()
        ck.red("grad_p", gp[keep], r64["gp"][keep], terms[keep], rows, al["px"] * xm + 2 * al["p2"] * pm + al["pa"] * am)
    if ga is not None:
        terms = r64["xa"].abs().t() @ x64.abs() + col("pa") * p64.abs() + col("an") * a64.abs() / an
        ck.red("grad_a", ga[keep], r64["ga"][keep], terms[keep], rows, al["xa"] * xm + al["pa"] * pm + al["an"] * float((a64.abs() / an).max()))
    if gs is not None:
        ck.red("grad_scale", gs, r64["gs"], r64["go_out"].abs().sum(0), rows, sc.grad_allowance(r64["go_out"], r32["go_out"]))


def _case(x, p, a, ls, go, signed, scaled, tag, key=None, rim=None, unaligned=False):
    """One case through the autograd function the layer and gmath.dist2plane share."""
    from hypad_amd.hyperspace import gmath
    rows, N = x.shape[0], p.shape[0]
    res = _refs(key, x, p, a, ls, go, signed, scaled)
    r64, r32 = res[F64], res[F32]
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, pd, ad = (mk(t).requires_grad_(True) for t in (x, p, a))
    ld = None if ls is None else ls.cuda().requires_grad_(True)
    flags = (SIGNED if signed else 0) | (SCALED if scaled else 0)
    out = gmath._Dist2Plane.apply(xd, pd, ad, ld, flags)
    out.backward(go.cuda())
    ck = Ck(tag)
    o, gx = out.detach().cpu(), xd.grad.cpu()
    if rim is not None:
        ck.cmp("out (rim row)", o[rim:rim + 1], r64["out"][rim:rim + 1], r32["out"][rim:rim + 1])
        ck.cmp("grad_x (rim row)", gx[rim:rim + 1], r64["gx"][rim:rim + 1], r32["gx"][rim:rim + 1])
        return ck
    kink = rows >= 3 and not signed                        # (the module docstring: row 0 on plane N // 2)
    ck.cmp("out", o, r64["out"], r32["out"])
    mask = None
    if kink:
        mask = np.ones(tuple(gx.shape), dtype=bool)
        mask[0] = False
    ck.cmp("grad_x", gx, r64["gx"], r32["gx"], mask=mask)
    _reductions(ck, res, x, p, a, rows, pd.grad.cpu(), ad.grad.cpu(), None if ls is None else ld.grad.cpu(), skip_plane=N // 2 if kink else None)
    for name, t in (("out", o), ("grad_x", gx), ("grad_p", pd.grad), ("grad_a", ad.grad), ("grad_scale", None if ls is None else ld.grad)):
        assert t is None or bool(torch.isfinite(t).all()), (tag, name)
    return ck


# ================================================================================================ the reference's recorded case
def test_recorded_cases_through_the_public_functions():
    from hypad_amd.hyperspace import gmath, hyrnn_nets
    from test_dist2plane_host import case_name, load_fixture
    fx = load_fixture()
    x, p, a, scale, go = (torch.from_numpy(fx[k]) for k in ("x", "p", "a", "scale", "grad_output"))
    cks = []
    for signed, scaled in ALL_FLAGS:
        name = case_name(signed, scaled)
        xd, pd, ad = (t.cuda().requires_grad_(True) for t in (x, p, a))
        out = gmath.dist2plane(xd.unsqueeze(-2), pd, ad, k=-1.0, signed=signed, scaled=scaled)
        assert out.shape == (9, 5)
        assert gmath.dist2plane(xd.unsqueeze(-2), pd, ad, signed=signed, scaled=scaled, keepdim=True).shape == (9, 5, 1)
        out.backward(go.cuda())
        res = _refs(None, x, p, a, None, go, signed, scaled)
        ck = Ck("recorded " + name)
        ck.cmp("out", out.detach().cpu(), res[F64]["out"], res[F32]["out"])
        mask = None
        if not signed:                                      # the fixture's row 7 lies on its plane 2
            mask = np.ones((9, 7), dtype=bool)
            mask[7] = False
        ck.cmp("grad_x", xd.grad.cpu(), res[F64]["gx"], res[F32]["gx"], mask=mask)
        _reductions(ck, res, x, p, a, 9, pd.grad.cpu(), ad.grad.cpu(), None, skip_plane=None if signed else 2)
        cks.append(ck)
    layer = hyrnn_nets.MobiusDist2Hyperplane(7, 5)
    with torch.no_grad():
        layer.point.copy_(p), layer.tangent.copy_(a), layer.scale.copy_(scale)
    layer = layer.cuda()
    xd = x.cuda().requires_grad_(True)
    out = layer(xd)
    out.backward(go.cuda())
    res = _refs(None, x, p, a, scale, go, True, False)
    ck = Ck("recorded layer")
    ck.cmp("out", out.detach().cpu(), res[F64]["out"], res[F32]["out"])
    ck.cmp("grad_x", xd.grad.cpu(), res[F64]["gx"], res[F32]["gx"])
    _reductions(ck, res, x, p, a, 9, layer.point.grad.cpu(), layer.tangent.grad.cpu(), layer.scale.grad.cpu())
    cks.append(ck)
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ the sweep
@pytest.mark.parametrize("rows,K,N", SHAPES)
def test_dist2plane_forward_and_backward(rows, K, N):
    """The layer's form (signed, not scaled, with log_scale) at every shape; the four flag combinations at (17, 33, 63) -- odd tails in
    rows, columns and planes -- and (65, 100, 100) -- two row tiles, two plane tiles -- without log_scale."""
    g = torch.Generator().manual_seed(10000 * rows + 100 * K + N)
    x, p, a, ls, go = _data(g, rows, K, N)
    cks = [_case(x, p, a, ls, go, True, False, f"({rows},{K},{N}) layer form")]
    if (rows, K, N) in ((17, 33, 63), (65, 100, 100)):
        for signed, scaled in ALL_FLAGS:
            cks.append(_case(x, p, a, None, go, signed, scaled, f"({rows},{K},{N}) signed={signed} scaled={scaled}"))
    _report(f"({rows},{K},{N})", cks)
    _finish(cks)


@pytest.mark.parametrize("rows,K,N", SHAPES)
def test_dist2plane_rim_row(rows, K, N):
    """One row on the 1 - 1e-3 norm, its out and grad_x rows compared alone (with it in the tensor, err32 of the whole tensor would be
    that row's).  err32 of such a single row is one draw from a wide distribution -- it depends on the order of the CPU's fp32 sums,
    i.e. on the machine's thread count: a first, all-fp32 form of the epilogue, which took 1 - n2 from the expansion of n2 as the
    restatement does, sat at 0.06 .. 0.91 of the allowance in one process and at 4.28 at (130,100,200) in another (errgpu
    9.3e-5 in grad_x against err32 2.5e-6; the kernel's result does not change between runs).  The kernels now take 1 - n2 from its closed form beta (1 - x2) / D with
    1 - x2 and beta from fp64 sums (dist2plane.hip), which leaves the row its digits whatever the yardstick draws."""
    g = torch.Generator().manual_seed(10000 * rows + 100 * K + N + 1)
    x, p, a, ls, go = _data(g, rows, K, N, rim=True)
    ck = _case(x, p, a, ls, go, True, False, f"({rows},{K},{N}) rim row", rim=1 if rows >= 3 else 0)
    _report(f"rim row ({rows},{K},{N})", [ck])
    _finish([ck])


def _many_rows():
    g = torch.Generator().manual_seed(4099)
    return _data(g, 4099, 100, 100)


def test_dist2plane_column_sums_across_many_row_tiles():
    """4 099 rows at (100, 100): 65 row tiles feed every column sum of grad_p / grad_a / grad_scale."""
    x, p, a, ls, go = _many_rows()
    ck = _case(x, p, a, ls, go, True, True, "(4099,100,100) signed, scaled", key="many")
    _report("4 099 rows", [ck])
    _finish([ck])


def test_two_backward_runs_give_the_same_bits():
    from hypad_amd.hyperspace import gmath
    x, p, a, ls, go = _many_rows()
    got = []
    for _ in range(2):
        xd, pd, ad, ld = (t.cuda().requires_grad_(True) for t in (x, p, a, ls))
        out = gmath._Dist2Plane.apply(xd, pd, ad, ld, SIGNED | SCALED)
        torch.full((4099 * 100 * 6,), NAN, device="cuda")   # (another history of the allocator's blocks between the runs)
        out.backward(go.cuda())
        got.append((out.detach(), xd.grad, pd.grad, ad.grad, ld.grad))
    for u, v in zip(*got):
        assert torch.equal(u, v)


def test_dist2plane_with_operands_at_storage_offset_1():
    g = torch.Generator().manual_seed(391001)
    x, p, a, ls, go = _data(g, 39, 100, 100)
    ck = _case(x, p, a, ls, go, True, False, "(39,100,100) layer form, x, p, a at storage offset 1", unaligned=True)
    _report("unaligned", [ck])
    _finish([ck])


# ================================================================================================ the C ABI directly
def _abi_case():
    g = torch.Generator().manual_seed(173363)
    rows, K, N = 17, 33, 63
    x, p, a, ls, go = _data(g, rows, K, N)
    return rows, K, N, x, p, a, ls, go


def test_out_and_grad_x_are_written_between_their_guards():
    c = _C()
    rows, K, N, x, p, a, ls, go = _abi_case()
    res = _refs("abi", x, p, a, ls, go, True, False)
    xd, pd, ad, ld, god = (t.cuda() for t in (x, p, a, ls, go))
    obuf, out = _guarded((rows, N), 3)
    gbuf, gx = _guarded((rows, K), 5)
    c.check(c.lib.hypad_dist2plane_fwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), c.ptr(ld), c.ptr(out), rows, K, N, SIGNED, c.stream()), "dist2plane_fwd")
    need = c.lib.hypad_dist2plane_workspace_bytes(rows, K, N)
    ws = torch.full((need // 4,), NAN, device="cuda")
    c.check(c.lib.hypad_dist2plane_bwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), c.ptr(ld), c.ptr(out), c.ptr(god), c.ptr(gx), None, None, None, c.ptr(ws),
                                       need, rows, K, N, SIGNED, c.stream()), "dist2plane_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, 3) and _guards_intact(gbuf, 5)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(gx).all())
    ck = Ck("guarded (17,33,63)")
    ck.cmp("out", out.cpu(), res[F64]["out"], res[F32]["out"])
    ck.cmp("grad_x", gx.cpu(), res[F64]["gx"], res[F32]["gx"])
    _finish([ck])


def test_each_null_gradient_combination():
    """Every subset of (grad_x, grad_p, grad_a, grad_log_scale): what is asked for has the bits of the run that asks for everything."""
    c = _C()
    rows, K, N, x, p, a, ls, go = _abi_case()
    xd, pd, ad, ld, god = (t.cuda() for t in (x, p, a, ls, go))
    out = torch.empty(rows, N, device="cuda")
    c.check(c.lib.hypad_dist2plane_fwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), c.ptr(ld), c.ptr(out), rows, K, N, SIGNED | SCALED, c.stream()), "dist2plane_fwd")
    need = c.lib.hypad_dist2plane_workspace_bytes(rows, K, N)
    shapes = ((rows, K), (N, K), (N, K), (N,))
    full = None
    for sel in range(15, -1, -1):
        ws = torch.full((need // 4,), NAN, device="cuda")
        outs = [torch.full(s, NAN, device="cuda") if sel >> i & 1 else None for i, s in enumerate(shapes)]
        c.check(c.lib.hypad_dist2plane_bwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), c.ptr(ld), c.ptr(out), c.ptr(god), *(c.ptr(t) for t in outs), c.ptr(ws),
                                           need, rows, K, N, SIGNED | SCALED, c.stream()), f"dist2plane_bwd {sel:04b}")
        if sel == 15:
            full = outs
            res = _refs("abi-scaled", x, p, a, ls, go, True, True)
            ck = Ck("C ABI (17,33,63) signed, scaled")
            ck.cmp("grad_x", outs[0].cpu(), res[F64]["gx"], res[F32]["gx"])
            _reductions(ck, res, x, p, a, rows, outs[1].cpu(), outs[2].cpu(), outs[3].cpu())
            _finish([ck])
        for t, f in zip(outs, full):
            assert t is None or torch.equal(t, f), f"{sel:04b}"
    # without a log_scale: its gradient cannot be asked for; the others run
    gx = torch.full((rows, K), NAN, device="cuda")
    ws = torch.full((need // 4,), NAN, device="cuda")
    assert c.lib.hypad_dist2plane_bwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), None, None, c.ptr(god), c.ptr(gx), None, None, c.ptr(out), c.ptr(ws), need,
                                      rows, K, N, SIGNED, c.stream()) == HYPAD_EINVAL
    assert c.lib.hypad_dist2plane_bwd(c.ptr(xd), c.ptr(pd), c.ptr(ad), None, None, c.ptr(god), c.ptr(gx), None, None, None, c.ptr(ws), need,
                                      rows, K, N, SIGNED, c.stream()) == 0
    assert bool(torch.isfinite(gx).all())


def test_refusals_write_nothing():
    c = _C()
    rows, N = 4, 16
    for K, want in ((257, HYPAD_EUNSUPPORTED), (8, None)):
        x, p, a, ls, go = (torch.zeros(s, device="cuda") for s in ((rows, K), (N, K), (N, K), (N,), (rows, N)))
        out, gx, gp, ga, gs = (torch.full(s, SENTINEL, device="cuda") for s in ((rows, N), (rows, K), (N, K), (N, K), (N,)))
        need = c.lib.hypad_dist2plane_workspace_bytes(rows, K, N)
        ws = torch.full((need // 4,), SENTINEL, device="cuda")
        fwd = lambda xx=x, pp=p, r=rows, k=K, n=N, f=SIGNED: c.lib.hypad_dist2plane_fwd(c.ptr(xx), c.ptr(pp), c.ptr(a), c.ptr(ls), c.ptr(out), r, k, n, f,
                                                                                        c.stream())
        bwd = lambda nbytes=need, xx=x, r=rows, k=K, n=N, f=SIGNED: c.lib.hypad_dist2plane_bwd(
            c.ptr(xx), c.ptr(p), c.ptr(a), c.ptr(ls), c.ptr(out), c.ptr(go), c.ptr(gx), c.ptr(gp), c.ptr(ga), c.ptr(gs), c.ptr(ws), nbytes, r, k, n, f, c.stream())
        if want is not None:                                # in_dim = 257
            assert fwd() == want and bwd() == want
        else:
            assert fwd(xx=None) == HYPAD_EINVAL and fwd(pp=None) == HYPAD_EINVAL and bwd(xx=None) == HYPAD_EINVAL
            assert fwd(r=-1) == HYPAD_EINVAL and fwd(k=0) == HYPAD_EINVAL and fwd(n=0) == HYPAD_EINVAL and fwd(f=4) == HYPAD_EINVAL
            assert bwd(r=-1) == HYPAD_EINVAL and bwd(k=0) == HYPAD_EINVAL and bwd(n=-3) == HYPAD_EINVAL and bwd(f=8) == HYPAD_EINVAL
            assert bwd(nbytes=need - 4) == HYPAD_EWORKSPACE
        torch.cuda.synchronize()
        for t in (out, gx, gp, ga, gs, ws):
            assert bool((t == SENTINEL).all())              # nothing ran
    assert fwd() == 0 and bwd() == 0
    from hypad_amd.hyperspace import gmath
    with pytest.raises(NotImplementedError, match="supported"):
        gmath.dist2plane(torch.zeros(4, 1, 257, device="cuda"), torch.zeros(5, 257, device="cuda"), torch.zeros(5, 257, device="cuda"))


def test_empty_batch_leaves_zero_parameter_gradients():
    from hypad_amd.hyperspace import hyrnn_nets
    layer = hyrnn_nets.MobiusDist2Hyperplane(33, 17).cuda()
    x = torch.empty(0, 33, device="cuda", requires_grad=True)
    out = layer(x)
    assert out.shape == (0, 17)
    poison = [torch.full(tuple(prm.shape), NAN, device="cuda") for prm in layer.parameters()]   # NaN into the allocator's free blocks of these sizes
    torch.cuda.synchronize()
    del poison
    out.sum().backward()
    for n, prm in layer.named_parameters():
        assert prm.grad is not None and prm.grad.shape == prm.shape and bool((prm.grad == 0).all()), n
    assert x.grad.shape == (0, 33)


# ================================================================================================ end to end
def test_two_mobius_linear_layers_and_the_read_out_take_an_sgd_step():
    """Euclidean -> ball (tanh) -> ball -> distances to 11 hyperplanes -> cross-entropy, one SGD step of every parameter."""
    from hypad_amd.hyperspace import hyrnn_nets
    from test_mobius_modes_host import mobius_linear_ref
    rows, K, H, M, N = 39, 33, 20, 17, 11
    g = torch.Generator().manual_seed(39332017)
    x = torch.randn(rows, K, generator=g)
    w1 = torch.randn(H, K, generator=g) * (0.25 / K ** 0.5)
    w2 = torch.randn(M, H, generator=g) * (1.0 / H ** 0.5)
    b1, b2 = _ball_rows(g, 1, H, radius=0.5)[0], _ball_rows(g, 1, M, radius=0.5)[0]
    point, tangent = _ball_rows(g, N, M, radius=0.8, edge=False, zero_row=False), torch.randn(N, M, generator=g)
    scale, target = 0.3 * torch.randn(N, generator=g), torch.randint(0, N, (rows,), generator=g)
    res = {}
    for dt in (F64, F32):
        xx, p = _leaf(x, dt), [_leaf(t, dt) for t in (w1, w2, point, tangent, scale)]
        br = [t.to(dt).unsqueeze(0).expand(rows, -1).clone().requires_grad_(True) for t in (b1, b2)]
        h1, _ = mobius_linear_ref(xx, p[0], br[0], False, True, torch.tanh)
        h2, _ = mobius_linear_ref(h1, p[1], br[1], True, True, None)
        logits, parts = dist2plane_parts(h2, p[2], p[3], True, False, p[4])
        loss = torch.nn.functional.cross_entropy(logits, target)
        go = torch.autograd.grad(loss, logits, retain_graph=True)[0]
        gs = torch.autograd.grad(logits, [xx, p[2], p[3], p[4]] + [parts[k] for k in PARTS], go)
        res[dt] = dict(out=logits.detach(), loss=loss.detach(), h2=h2.detach(), gx=gs[0], gp=gs[1], ga=gs[2], gs=gs[3], go_out=go * logits.detach(),
                       **{k: c for k, c in zip(PARTS, gs[4:])})
    r64, r32 = res[F64], res[F32]
    l1 = hyrnn_nets.MobiusLinear(K, H, hyperbolic_input=False, nonlin=torch.tanh, fp64_hyper=False)
    l2 = hyrnn_nets.MobiusLinear(H, M, fp64_hyper=False)
    head = hyrnn_nets.MobiusDist2Hyperplane(M, N)
    with torch.no_grad():
        for lay, w, b in ((l1, w1, b1), (l2, w2, b2)):
            lay.weight.copy_(w), lay.bias.copy_(b)
        head.point.copy_(point), head.tangent.copy_(tangent), head.scale.copy_(scale)
    net = torch.nn.Sequential(l1, l2, head).cuda()
    params = list(net.parameters())
    assert len(params) == 7
    before = [q.detach().clone() for q in params]
    opt = torch.optim.SGD(params, lr=0.1)
    xd = x.cuda().requires_grad_(True)
    logits = net(xd)
    loss = torch.nn.functional.cross_entropy(logits, target.cuda())
    loss.backward()
    ck = Ck(f"MobiusLinear {K} -> {H} -> {M} -> MobiusDist2Hyperplane {N}, rows {rows}")
    ck.cmp("logits", logits.detach().cpu(), r64["out"], r32["out"])
    ck.cmp("loss", loss.detach().cpu(), r64["loss"], r32["loss"])
    ck.cmp("grad_x", xd.grad.cpu(), r64["gx"], r32["gx"])
    _reductions(ck, res, r64["h2"], point, tangent, rows, head.point.grad.cpu(), head.tangent.grad.cpu(), head.scale.grad.cpu())
    opt.step()
    for q, q0 in zip(params, before):
        assert not torch.equal(q, q0) and torch.equal(q.detach(), torch.add(q0, q.grad, alpha=-0.1))
    _report("end to end", [ck])
    _finish([ck])
