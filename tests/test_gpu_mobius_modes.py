"""mobius_linear in every configuration and the Moebius matvec on the GPU (hypad_mobius_linear_ex_*, hypad_mobius_matvec_*;
hyperspace/hyrnn_nets.py runs them) against the plain-torch restatement of tests/test_mobius_modes_host.py -- which that file pins to
the reference's own outputs -- run in fp64 and fp32 on the CPU, under the two rules of tests/test_gpu_dense_layers.py: per-row
quantities (out, the saved mx = x W^T, grad_x) under ``Ck.cmp``, sums over rows (grad_weight, grad_bias) under ``Ck.red`` with the
summand allowances of that file's ``_mobius_linear_case``.  No tolerance of its own.

The sweep's rows lie within radius 0.9 (``_ball_rows(..., radius=0.9, edge=False)``), the last one all zero: the reference's ``cond``
-- with a ball-valued input its mx is exactly zero, its output is exactly zero where nothing is added to it, and its grad_x is exactly
zero.  A row on the 1 - 1e-3 norm is compared in a ``cmp`` call of its own, forward and grad_x, in a test of its own
(``test_mobius_modes_rim_row``).
"""
import numpy as np
import pytest
import torch

import sweep_common as sc
from sweep_common import NAN, SENTINEL, Ck, _ball_rows, _leaf, _unaligned
from test_mobius_modes_host import CASES, NONLINS, case_name, load_fixture, mobius_linear_ref, mobius_matvec_ref

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EWORKSPACE, HYPAD_EUNSUPPORTED = -1, -2, -3          # include/hypad.h
# (hyperbolic_input, hyperbolic_bias, with bias)
MODES = {"ball input, ball bias": (True, True, True), "ball input, Euclidean bias": (True, False, True),
         "ball input, no bias": (True, True, False), "Euclidean input, Euclidean bias": (False, False, True)}
MOBIUS_KN = [(1, 1), (3, 5), (33, 63), (64, 64), (100, 100), (129, 65), (51, 256), (256, 256)]


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\nmobius modes {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")


def _data(g, rows, K, N, rim=False):
    """x: rows inside the ball at radius <= 0.9, the last one all zero (rows >= 2); rim=True: row 1 on the 1 - 1e-3 norm (rows >= 3);
    the weight scaled so that max |x W^T| / |x| = 1.5; a bias of norm <= 0.5 (a point of the ball, or the tangent vector expmap0
    maps); grad_output ~ N(0, 1)."""
    x = _ball_rows(g, rows, K, radius=0.9, edge=False).double()
    if rows >= 3 and rim:
        x[1] *= (1 - 1e-3) / float(x[1].norm())
    w = torch.randn(N, K, generator=g, dtype=F64)
    xn = x.norm(dim=1)
    live = xn > 0
    ratio = ((x @ w.t()).norm(dim=1)[live] / xn[live]).max() if bool(live.any()) else torch.tensor(1.0)
    w = w * (1.5 / float(ratio))
    b = _ball_rows(g, 1, N, radius=0.5)[0]
    return x.float(), w.float(), b, torch.randn(rows, N, generator=g)


def _refs(x, w, b, go, hi, hb, nl):
    rows = x.shape[0]
    res = {}
    for dt in (F64, F32):
        xx, ww = _leaf(x, dt), _leaf(w, dt)
        bb = None if b is None else b.to(dt).unsqueeze(0).expand(rows, -1).clone().requires_grad_(True)
        o, mx = mobius_linear_ref(xx, ww, bb, hi, hb, NONLINS[nl])
        gs = torch.autograd.grad(o, [xx, ww, mx] + ([] if b is None else [bb]), go.to(dt))
        res[dt] = dict(out=o.detach(), mx=mx.detach(), gx=gs[0], gw=gs[1], gmx=gs[2], gbr=None if b is None else gs[3])
    return res


def _reductions(ck, res, x, rows, gw, gb):
    r64, r32 = res[F64], res[F32]
    x64 = x.double()
    ck.red("grad_weight", gw, r64["gw"], r64["gmx"].abs().t() @ x64.abs(), rows,
           sc.grad_allowance(r64["gmx"], r32["gmx"]) * float(x64.abs().max()))
    if gb is not None:
        ck.red("grad_bias", gb, r64["gbr"].sum(0), r64["gbr"].abs().sum(0), rows, sc.grad_allowance(r64["gbr"], r32["gbr"]))


def _case(x, w, b, go, hi, hb, nl, tag, rim=None, unaligned=False, only_grad_x=False):
    """One configuration through hyrnn_nets.mobius_linear: forward, saved mx and the three gradients.  rim: only that row's out and
    grad_x, each in a cmp call of its own."""
    from hypad_amd.hyperspace import hyrnn_nets
    rows = x.shape[0]
    res = _refs(x, w, b, go, hi, hb, nl)
    r64, r32 = res[F64], res[F32]
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, wd = mk(x).requires_grad_(True), mk(w).requires_grad_(True)
    bd = None if b is None else b.cuda().requires_grad_(True)
    out = hyrnn_nets.mobius_linear(xd, wd, bd, hyperbolic_input=hi, hyperbolic_bias=hb, nonlin=NONLINS[nl])
    mx_saved = out.grad_fn.saved_tensors[2] if type(out.grad_fn).__name__.startswith("_MobiusLinearExFn") else None
    out.backward(go.cuda())
    ck = Ck(tag)
    gx, o = xd.grad.cpu(), out.detach().cpu()
    if rim is not None:
        ck.cmp("out (rim row)", o[rim:rim + 1], r64["out"][rim:rim + 1], r32["out"][rim:rim + 1])
        ck.cmp("grad_x (rim row)", gx[rim:rim + 1], r64["gx"][rim:rim + 1], r32["gx"][rim:rim + 1])
        return ck
    ck.cmp("grad_x", gx, r64["gx"], r32["gx"])
    if only_grad_x:
        return ck
    ck.cmp("out", o, r64["out"], r32["out"])
    if mx_saved is not None:                                  # (the configuration of models/tadgan.py keeps its own function)
        ck.cmp("saved mx", mx_saved.cpu(), r64["mx"], r32["mx"])
    _reductions(ck, res, x, rows, wd.grad.cpu(), None if b is None else bd.grad.cpu())
    for name, t in (("out", o), ("grad_x", gx), ("grad_weight", wd.grad), ("grad_bias", None if b is None else bd.grad)):
        assert t is None or bool(torch.isfinite(t).all()), (tag, name)
    zero = bool((x[-1] == 0).all()) and rows >= 2
    if zero and hi:                                           # `cond`
        assert bool((gx[-1] == 0).all()), (tag, "grad_x of the all-zero row")
        assert bool((r64["out"][-1] == 0).all()) == bool((o[-1] == 0).all()), (tag, "out of the all-zero row")
        if b is None:
            assert bool((o[-1] == 0).all()), (tag, "out of the all-zero row")
    return ck


# ================================================================================================ the reference's recorded cases
def test_every_recorded_configuration_through_the_public_functions():
    from hypad_amd.hyperspace import hyrnn_nets
    fx = load_fixture()
    x, w, go = (torch.from_numpy(fx[k]) for k in ("x", "weight", "grad_output"))
    cks = []
    for hi, hb, wb, nl in CASES:
        b = torch.from_numpy(fx["bias_ball" if hb else "bias_eucl"]) if wb else None
        cks.append(_case(x, w, b, go, hi, hb, nl, "recorded " + case_name(hi, hb, wb, nl)))
    # the bare matvec: hyrnn_nets.mobius_matvec
    res = {}
    for dt in (F64, F32):
        xx, ww = _leaf(x, dt), _leaf(w, dt)
        o, mx = mobius_matvec_ref(ww, xx)
        gx, gw, gmx = torch.autograd.grad(o, [xx, ww, mx], go.to(dt))
        res[dt] = dict(out=o.detach(), gx=gx, gw=gw, gmx=gmx, gbr=None)
    xd, wd = x.cuda().requires_grad_(True), w.cuda().requires_grad_(True)
    out = hyrnn_nets.mobius_matvec(wd, xd, k=-1.0)
    out.backward(go.cuda())
    ck = Ck("recorded matvec")
    ck.cmp("out", out.detach().cpu(), res[F64]["out"], res[F32]["out"])
    ck.cmp("grad_x", xd.grad.cpu(), res[F64]["gx"], res[F32]["gx"])
    _reductions(ck, res, x, x.shape[0], wd.grad.cpu(), None)
    assert bool((out[3] == 0).all()) and bool((xd.grad[3] == 0).all())
    cks.append(ck)
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ the sweep
@pytest.mark.parametrize("K,N", MOBIUS_KN)
def test_mobius_modes_forward_and_backward(K, N):
    g = torch.Generator().manual_seed(100 * K + N + 7)
    cks = []
    for rows in (1, 17, 39):
        x, w, b, go = _data(g, rows, K, N)
        for mode, (hi, hb, wb) in MODES.items():
            for nl in NONLINS:
                cks.append(_case(x, w, b if wb else None, go, hi, hb, nl, f"({K},{N}) rows {rows} {mode}, {nl}"))
    _report(f"({K},{N})", cks)
    _finish(cks)


@pytest.mark.parametrize("K,N", MOBIUS_KN)
def test_mobius_modes_rim_row(K, N):
    """Row 1 of a five-row input sits on the 1 - 1e-3 norm; its out and grad_x rows are compared alone, each in a cmp call of its own
    (with the rim row in a tensor, err32 of the whole tensor is that row's: 1e-5 .. 2e-3 against 3e-6 for rows within radius 0.9).

    The matvec scaling sends that row to norm tanh(ratio * artanh(0.999)) = 1 - 1e-5 .. 1 - 1e-3, and what follows takes 1 - norm
    from the row again.  err32 of such a single row is one draw from a wide distribution -- the fp32 restatement on the CPU with the
    columns of x / weight / bias permuted (the same numbers summed in another order) spreads over 5.6e-06 .. 5.4e-04 in grad_x where
    err32 is 8.0e-06 -- so a chain in fp32 passes or fails here by the order of its sums (a first, fp32 form of the kernels: 0.10 ..
    4.49 of the allowance over the eight shapes).  The kernels carry the row chain in fp64 registers for that reason (rowops.h) and
    sit at 0.005 .. 0.134 of the allowance."""
    g = torch.Generator().manual_seed(100 * K + N + 11)
    x, w, b, go = _data(g, 5, K, N, rim=True)
    cks = []
    for mode, (hi, hb, wb) in MODES.items():
        for nl in NONLINS:
            cks.append(_case(x, w, b if wb else None, go, hi, hb, nl, f"({K},{N}) rows 5 {mode}, {nl}", rim=1))
    _report(f"rim row ({K},{N})", cks)
    _finish(cks)


def test_mobius_modes_with_unaligned_input_and_weight():
    """(64, 64) x 39 with x and weight at storage offset 1: the scalar weight loads of gemm_nt and the scalar tile stores."""
    g = torch.Generator().manual_seed(6464)
    x, w, b, go = _data(g, 39, 64, 64)
    ck = _case(x, w, b, go, True, False, "tanh", "(64,64) rows 39 ball input, Euclidean bias, tanh, unaligned", unaligned=True)
    _report("unaligned", [ck])
    _finish([ck])


def test_mobius_modes_row_backward_beyond_one_grid_stride():
    """66 133 rows at (100, 100): more than the 16 384 rows one grid of the row backward (and of the norm-gradient pass) covers."""
    g = torch.Generator().manual_seed(66133)
    x, w, b, go = _data(g, 66133, 100, 100)
    ck = _case(x, w, b, go, True, True, "tanh", "(100,100) rows 66133 ball input, ball bias, tanh", only_grad_x=True)
    _report("66 133 rows", [ck])
    _finish([ck])


def test_mobius_matvec_entry_points_directly():
    """hypad_mobius_matvec_fwd / _bwd at (33, 63) x 17."""
    c = _C()
    rows, K, N = 17, 33, 63
    g = torch.Generator().manual_seed(3363)
    x, w, _, go = _data(g, rows, K, N)
    res = {}
    for dt in (F64, F32):
        xx, ww = _leaf(x, dt), _leaf(w, dt)
        o, mx = mobius_matvec_ref(ww, xx)
        gx, gw, gmx = torch.autograd.grad(o, [xx, ww, mx], go.to(dt))
        res[dt] = dict(out=o.detach(), mx=mx.detach(), gx=gx, gw=gw, gmx=gmx, gbr=None)
    r64, r32 = res[F64], res[F32]
    xd, wd, god = x.cuda(), w.cuda(), go.cuda()
    out, mx, gx, gw = (torch.full(s, NAN, device="cuda") for s in ((rows, N), (rows, N), (rows, K), (N, K)))
    c.check(c.lib.hypad_mobius_matvec_fwd(c.ptr(xd), c.ptr(wd), c.ptr(out), c.ptr(mx), rows, K, N, c.stream()), "mobius_matvec_fwd")
    need = c.lib.hypad_mobius_linear_ex_workspace_bytes(rows, N)
    ws = torch.full((need // 4,), NAN, device="cuda")
    c.check(c.lib.hypad_mobius_matvec_bwd(c.ptr(xd), c.ptr(wd), c.ptr(mx), c.ptr(god), c.ptr(gx), c.ptr(gw), c.ptr(ws), need, rows, K, N,
                                          c.stream()), "mobius_matvec_bwd")
    ck = Ck(f"mobius_matvec ({K},{N}) rows {rows}")
    ck.cmp("out", out.cpu(), r64["out"], r32["out"])
    ck.cmp("saved mx", mx.cpu(), r64["mx"], r32["mx"])
    ck.cmp("grad_x", gx.cpu(), r64["gx"], r32["gx"])
    _reductions(ck, res, x, rows, gw.cpu(), None)
    assert bool((out[-1] == 0).all()) and bool((gx[-1] == 0).all())
    # the forward without mx_save, the backward without grad_x: the same bits
    out2, gw2 = torch.full((rows, N), NAN, device="cuda"), torch.full((N, K), NAN, device="cuda")
    c.check(c.lib.hypad_mobius_matvec_fwd(c.ptr(xd), c.ptr(wd), c.ptr(out2), None, rows, K, N, c.stream()), "mobius_matvec_fwd")
    c.check(c.lib.hypad_mobius_matvec_bwd(c.ptr(xd), c.ptr(wd), c.ptr(mx), c.ptr(god), None, c.ptr(gw2), c.ptr(ws), need, rows, K, N,
                                          c.stream()), "mobius_matvec_bwd")
    assert torch.equal(out, out2) and torch.equal(gw, gw2)
    _report("matvec entry points", [ck])
    _finish([ck])


def test_gmath_mobius_fn_apply_and_mobius_matvec():
    """gmath.mobius_fn_apply(fn, x) = expmap0(fn(logmap0(x))) over the two HIP maps, forward and grad_x, for tanh, relu and a function
    the fused layer does not take; gmath.mobius_matvec is hyrnn_nets.mobius_matvec."""
    from hypad_amd.hyperspace import gmath
    from test_mobius_modes_host import mobius_fn_apply_ref
    g = torch.Generator().manual_seed(77)
    x, go = _ball_rows(g, 39, 100, radius=0.9, edge=False), torch.randn(39, 100, generator=g)
    cks = []
    for name, fn in (("tanh", torch.tanh), ("relu", torch.relu), ("sigmoid", torch.sigmoid)):
        res = {}
        for dt in (F64, F32):
            xx = _leaf(x, dt)
            o = mobius_fn_apply_ref(fn, xx)
            res[dt] = (o.detach(), torch.autograd.grad(o, xx, go.to(dt))[0])
        xd = x.cuda().requires_grad_(True)
        out = gmath.mobius_fn_apply(fn, xd, k=-1.0)
        out.backward(go.cuda())
        ck = Ck(f"mobius_fn_apply {name} (39, 100)")
        ck.cmp("out", out.detach().cpu(), res[F64][0], res[F32][0])
        ck.cmp("grad_x", xd.grad.cpu(), res[F64][1], res[F32][1])
        cks.append(ck)
    w = torch.randn(17, 100, generator=g) * 0.1
    from hypad_amd.hyperspace import hyrnn_nets
    assert torch.equal(gmath.mobius_matvec(w.cuda(), x.cuda(), k=-1.0), hyrnn_nets.mobius_matvec(w.cuda(), x.cuda(), k=-1.0))
    _report("gmath.mobius_fn_apply", cks)
    _finish(cks)


# ================================================================================================ refusals and the empty batch
def test_mobius_modes_refuse_width_257_and_a_short_workspace():
    c = _C()
    rows, K = 4, 8
    x, w257, b257 = torch.zeros(rows, K, device="cuda"), torch.zeros(257, K, device="cuda"), torch.zeros(257, device="cuda")
    out = torch.full((rows, 257), SENTINEL, device="cuda")
    assert c.lib.hypad_mobius_linear_ex_fwd(c.ptr(x), c.ptr(w257), c.ptr(b257), c.ptr(out), None, rows, K, 257, 3, 1, c.stream()) == HYPAD_EUNSUPPORTED
    assert c.lib.hypad_mobius_matvec_fwd(c.ptr(x), c.ptr(w257), c.ptr(out), None, rows, K, 257, c.stream()) == HYPAD_EUNSUPPORTED
    N = 16
    w, b, mx, go = (torch.zeros(s, device="cuda") for s in ((N, K), (N,), (rows, N), (rows, N)))
    gx, gw, gb = (torch.full(s, SENTINEL, device="cuda") for s in ((rows, K), (N, K), (N,)))
    need = c.lib.hypad_mobius_linear_ex_workspace_bytes(rows, N)
    assert need == (2 * rows * N + rows + N) * 4
    ws = torch.full((need // 4,), SENTINEL, device="cuda")
    args = lambda nbytes, n=N: (c.ptr(x), c.ptr(w), c.ptr(b), c.ptr(mx), c.ptr(go), c.ptr(gx), c.ptr(gw), c.ptr(gb), c.ptr(ws), nbytes, rows, K, n,
                                3, 1, c.stream())
    assert c.lib.hypad_mobius_linear_ex_bwd(*args(need - 4)) == HYPAD_EWORKSPACE
    assert c.lib.hypad_mobius_matvec_bwd(c.ptr(x), c.ptr(w), c.ptr(mx), c.ptr(go), c.ptr(gx), c.ptr(gw), c.ptr(ws), need - 4, rows, K, N,
                                         c.stream()) == HYPAD_EWORKSPACE
    assert c.lib.hypad_mobius_linear_ex_bwd(*args(1 << 20, 257)) == HYPAD_EUNSUPPORTED
    assert c.lib.hypad_mobius_linear_ex_bwd(*args(need)[:-3], 4, 1, c.stream()) == HYPAD_EINVAL          # an unknown flag bit
    assert c.lib.hypad_mobius_linear_ex_bwd(*args(need)[:-2], 3, c.stream()) == HYPAD_EINVAL             # an unknown non-linearity
    torch.cuda.synchronize()
    for t in (out, gx, gw, gb, ws):
        assert bool((t == SENTINEL).all())                                                                # nothing ran
    assert c.lib.hypad_mobius_linear_ex_bwd(*args(need)) == 0


def test_empty_batch_through_the_mobius_modes_leaves_zero_parameter_gradients():
    from hypad_amd.hyperspace import hyrnn_nets
    w = torch.randn(17, 33, device="cuda", requires_grad=True)
    b = (0.01 * torch.randn(17, device="cuda")).requires_grad_(True)
    x = torch.empty(0, 33, device="cuda", requires_grad=True)
    out = hyrnn_nets.mobius_linear(x, w, b, hyperbolic_input=True, hyperbolic_bias=False, nonlin=torch.relu)
    assert out.shape == (0, 17)
    poison = [torch.full(tuple(s), NAN, device="cuda") for s in (w.shape, b.shape)]    # NaN into the allocator's free blocks of these sizes
    torch.cuda.synchronize()
    del poison
    out.sum().backward()
    for n, p in (("weight", w), ("bias", b)):
        assert p.grad is not None and p.grad.shape == p.shape and bool((p.grad == 0).all()), n
    assert x.grad.shape == (0, 33)
    w2 = torch.randn(17, 33, device="cuda", requires_grad=True)
    assert hyrnn_nets.mobius_matvec(w2, x, k=-1.0).shape == (0, 17)
    hyrnn_nets.mobius_matvec(w2, x, k=-1.0).sum().backward()
    assert bool((w2.grad == 0).all())


def test_unsupported_arguments_still_raise_and_name_what_is_supported():
    from hypad_amd.hyperspace import hyrnn_nets
    x, w, b = torch.zeros(4, 8, device="cuda"), torch.zeros(5, 8, device="cuda"), torch.zeros(5, device="cuda")
    for call in (lambda: hyrnn_nets.mobius_linear(x, w, b, nonlin=torch.sigmoid),
                 lambda: hyrnn_nets.mobius_linear(x, w, b, k=-0.5),
                 lambda: hyrnn_nets.mobius_matvec(w, x, k=-1.0, dim=0),
                 lambda: hyrnn_nets.mobius_matvec(w.unsqueeze(0), x, k=-1.0),
                 lambda: hyrnn_nets.mobius_matvec(w, x, k=1.0),
                 lambda: hyrnn_nets.MobiusLinear(8, 5, fp64_hyper=True)):
        with pytest.raises(NotImplementedError, match="supported|fp64_hyper"):
            call()


# ================================================================================================ stacked layers, the old path
def test_two_stacked_mobius_linear_layers_take_an_sgd_step():
    """Euclidean -> ball (tanh) -> ball: the second layer has hyperbolic_input=True, the reference's default."""
    from hypad_amd.hyperspace import hyrnn_nets
    rows, K, H, N = 39, 33, 20, 17
    g = torch.Generator().manual_seed(332017)
    x = torch.randn(rows, K, generator=g)
    w1 = torch.randn(H, K, generator=g) * (0.25 / K ** 0.5)          # |x W1^T| ~ 1.1: expmap0 stays off the rim
    w2 = torch.randn(N, H, generator=g) * (1.0 / H ** 0.5)
    b1, b2 = _ball_rows(g, 1, H, radius=0.5)[0], _ball_rows(g, 1, N, radius=0.5)[0]
    go = torch.randn(rows, N, generator=g)
    res = {}
    for dt in (F64, F32):
        xx, p = _leaf(x, dt), [_leaf(t, dt) for t in (w1, w2)]
        br = [t.to(dt).unsqueeze(0).expand(rows, -1).clone().requires_grad_(True) for t in (b1, b2)]
        h, mx1 = mobius_linear_ref(xx, p[0], br[0], False, True, torch.tanh)
        o, mx2 = mobius_linear_ref(h, p[1], br[1], True, True, None)
        gs = torch.autograd.grad(o, [xx, p[0], p[1], br[0], br[1], mx1, mx2, h], go.to(dt))
        res[dt] = dict(out=o.detach(), h=h.detach(), gx=gs[0], gw=(gs[1], gs[2]), gbr=(gs[3], gs[4]), gmx=(gs[5], gs[6]), gh=gs[7])
    r64, r32 = res[F64], res[F32]
    l1 = hyrnn_nets.MobiusLinear(K, H, hyperbolic_input=False, nonlin=torch.tanh, fp64_hyper=False)
    l2 = hyrnn_nets.MobiusLinear(H, N, fp64_hyper=False)
    assert l2.hyperbolic_input and list(l1.state_dict()) == ["weight", "bias"]
    with torch.no_grad():
        for lay, w, b in ((l1, w1, b1), (l2, w2, b2)):
            lay.weight.copy_(w)
            lay.bias.copy_(b)
    l1, l2 = l1.cuda(), l2.cuda()
    params = list(l1.parameters()) + list(l2.parameters())
    before = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=0.1)
    xd = x.cuda().requires_grad_(True)
    out = l2(l1(xd))
    out.backward(go.cuda())
    ck = Ck(f"stacked MobiusLinear {K} -> {H} -> {N} rows {rows}")
    ck.cmp("out", out.detach().cpu(), r64["out"], r32["out"])
    ck.cmp("grad_x", xd.grad.cpu(), r64["gx"], r32["gx"])
    ins64 = (x.double(), r64["h"])
    for i, lay in enumerate((l1, l2)):
        a64 = ins64[i]
        ck.red(f"layer {i + 1} grad_weight", lay.weight.grad.cpu(), r64["gw"][i], r64["gmx"][i].abs().t() @ a64.abs(), rows,
               sc.grad_allowance(r64["gmx"][i], r32["gmx"][i]) * float(a64.abs().max()))
        ck.red(f"layer {i + 1} grad_bias", lay.bias.grad.cpu(), r64["gbr"][i].sum(0), r64["gbr"][i].abs().sum(0), rows,
               sc.grad_allowance(r64["gbr"][i], r32["gbr"][i]))
    opt.step()
    for p, p0 in zip(params, before):
        assert not torch.equal(p, p0) and torch.equal(p.detach(), torch.add(p0, p.grad, alpha=-0.1))
    _report("stacked layers", [ck])
    _finish([ck])


def test_the_existing_configuration_keeps_its_bits_through_the_dispatch():
    from hypad_amd.hyperspace import hyrnn_nets
    g = torch.Generator().manual_seed(5)
    x, w, b, go = torch.randn(39, 100, generator=g), torch.randn(100, 100, generator=g) * 0.02, _ball_rows(g, 1, 100, radius=0.5)[0], torch.randn(39, 100, generator=g)
    got = []
    for fn in (lambda a, ww, bb: hyrnn_nets.mobius_linear(a, ww, bb, hyperbolic_input=False, hyperbolic_bias=True, nonlin=None, k=-1.0),
               hyrnn_nets._MobiusLinearFn.apply):
        xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
        out = fn(xd, wd, bd)
        assert type(out.grad_fn).__name__.startswith("_MobiusLinearFn")
        out.backward(go.cuda())
        got.append((out.detach(), xd.grad, wd.grad, bd.grad))
    for a, b_ in zip(*got):
        assert torch.equal(a, b_)
