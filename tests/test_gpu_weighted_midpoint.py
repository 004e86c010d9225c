"""The weighted Moebius gyromidpoint in both forms and mobius_scalar_mul on the GPU (hypad_weighted_midpoint_*,
hypad_weighted_midpoint_bmm_*, hypad_mobius_scalar_mul_*; hyperspace/gmath runs them) against the plain-torch restatement of
tests/midpoint_ref.py -- which tests/test_weighted_midpoint_host.py pins to the reference's own outputs -- run in fp64 and fp32 on the
CPU, under the project's rule ``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1) for everything per element or per row, and
under ``Ck.red`` for the two sums over rows: grad_w of a single weight and grad_r of a single r.  No tolerance of its own.

The reductions.  A single weight's gradient is the sum over the M R (position, kept row) pairs of the gradient the pair's own weight
would get; the restatement run with the weight expanded to (M, R) gives those summands, ``abs_terms`` is the fp64 sum of their absolute
values and the summand allowance is their own ``grad_allowance`` (fp32 restatement against fp64).  The same for a single r over the rows.

The data.  Points: ``_ball_rows`` (radius <= 0.95, the last row all zero, no rim row).  bmm weights: a softmax over M of N(0, 1) scores,
or signed N(0, 1) * 2 / M (so that lincomb's alpha = sum |w| stays near 1.6 and tanh(alpha artanh |a|) is live); reduce weights:
U(0.1, 1) * 2 / M, U(-1, 1) * 2 / M, or the single weight 1.4 / M.  grad_out ~ N(0, 1).  A point on the 1 - 1e-3 norm feeds every
output of its batch element or kept row, so it gets a test of its own per shape (``test_*_rim_point``) and does not set err32 for the
others.

Tile and chunk sizes of the kernels (csrc/midpoint.hip), each with a shape at, one below and one above it in ``BMM_EDGES``:
    N: 64 output rows per workgroup            (1,63,20,20) (1,64,100,64) (1,65,20,20)   -- and 16 rows per wave: 15, 16, 17 via (3,17,33,20)
    M: 64 positions per chunk                  (1,20,63,20) (1,20,64,20) (1,20,65,20), two full chunks and a tail: (2,65,129,100)
    D: accumulator classes 64 / 128 / 256      (1,20,20,63) (1,64,100,64) (1,20,20,65) (1,20,20,127) (1,20,20,128) (1,20,20,129) (1,16,260,256)
    grad_w: 64 x 64 tiles, D in chunks of 128  the N, M shapes above; (1,20,20,127..129), (1,16,260,256) = two chunks
    grad_x: the forward's kernel with N and M exchanged: (1,63..65,20,20) are its chunk edges, (1,20,63..65,20) its row-tile edges
The reduce form has no tile: a wave per kept row, 64 lanes x 4 elements (D = 63, 100, 256 cover one to four elements a lane); its one
threshold is the slice count, 1 024 // R capped by M // 16 and 256: one slice at (2,4099,7) and (9,6,5), 7 at (100,64,100), 242 at (4099,1,20).
"""
import numpy as np
import pytest
import torch

import sweep_common as sc
from midpoint_ref import mobius_scalar_mul_ref, weighted_midpoint_bmm_ref, weighted_midpoint_ref
from sweep_common import NAN, SENTINEL, Ck, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EWORKSPACE, HYPAD_EUNSUPPORTED = -1, -2, -3          # include/hypad.h
LINCOMB, POSWEIGHT, COADD = 1, 2, 4                                        # HYPAD_MID_*
BMM_SHAPES = [(1, 1, 1, 1), (2, 5, 7, 3), (3, 17, 33, 20), (1, 64, 100, 64), (2, 65, 129, 100), (1, 16, 260, 256)]   # (batch, N, M, D)
BMM_EDGES = [(1, 63, 20, 20), (1, 65, 20, 20), (1, 20, 63, 20), (1, 20, 64, 20), (1, 20, 65, 20), (1, 20, 20, 63), (1, 20, 20, 65),
             (1, 20, 20, 127), (1, 20, 20, 128), (1, 20, 20, 129)]
RED_SHAPES = [(1, 1, 1), (9, 6, 5), (33, 17, 63), (100, 64, 100), (7, 3, 256), (4099, 1, 20), (2, 4099, 7)]           # (M, R, D)
# (weights, flags): every flag, every kind of weights
RED_CONFIGS = [(None, {}), (None, dict(lincomb=True)), ("scalar", {}), ("scalar", dict(lincomb=True)), ("pos", {}), ("pos", dict(lincomb=True)),
               ("signed", {}), ("signed", dict(posweight=True)), ("signed", dict(lincomb=True)), ("signed", dict(posweight=True, lincomb=True)),
               ("signed", dict(coadd=True)), ("scalarneg", dict(posweight=True, lincomb=True))]


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
    print(f"\nweighted midpoint {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")


def _rim(x2d, g):
    """One row of a (rows, D) matrix moved to the 1 - 1e-3 norm (a zero row gets a direction first)."""
    i = 1 if x2d.shape[0] >= 3 else 0
    v = x2d[i].double()
    if float(v.norm()) == 0:
        v = torch.randn(v.shape, generator=g, dtype=F64)
    x2d[i] = (v * ((1 - 1e-3) / float(v.norm()))).float()
    return x2d


# ================================================================================================ bmm form
def _bmm_data(batch, N, M, D, kind, rim=False, seed=0):
    g = torch.Generator().manual_seed(1000003 * batch + 10007 * N + 101 * M + D + seed)
    xs = _ball_rows(g, batch * M, D, edge=False)
    if rim:
        xs = _rim(xs, g)
    xs = xs.reshape(batch, M, D)
    s = torch.randn(batch, N, M, generator=g)
    w = torch.softmax(s, dim=-1) if kind == "softmax" else s * (2.0 / M)
    return xs, w.float(), torch.randn(batch, N, D, generator=g)


_REFS = {}


def _bmm_refs(key, xs, w, go, lincomb):
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        x, ww = _leaf(xs, dt), _leaf(w, dt)
        o = weighted_midpoint_bmm_ref(x, ww, lincomb=lincomb)
        gx, gw = torch.autograd.grad(o, [x, ww], go.to(dt))
        res[dt] = dict(out=o.detach(), gx=gx, gw=gw)
    if key is not None:
        _REFS[key] = res
    return res


def _bmm_run(xs, w, go, lincomb, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, wd = mk(xs).requires_grad_(True), mk(w).requires_grad_(True)
    out = _gmath().weighted_midpoint_bmm(xd, wd, -1.0, lincomb=lincomb)
    out.backward(go.cuda())
    return out.detach(), xd.grad, wd.grad


def _bmm_case(shape, kind, lincomb, tag, rim=False, key=None):
    xs, w, go = _bmm_data(*shape, kind, rim=rim)
    res = _bmm_refs(key, xs, w, go, lincomb)
    out, gx, gw = _bmm_run(xs, w, go, lincomb)
    ck = Ck(f"bmm {shape} {kind} lincomb={lincomb} {tag}")
    for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_w", gw, "gw")):
        assert bool(torch.isfinite(t).all()), (ck.case, name)
        ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
    return ck


@pytest.mark.parametrize("shape", BMM_SHAPES + BMM_EDGES, ids=lambda s: "x".join(map(str, s)))
def test_bmm_forward_and_backward(shape):
    cks = [_bmm_case(shape, kind, lincomb, "") for kind in ("softmax", "signed") for lincomb in (False, True)]
    _report(f"bmm {shape}", cks)
    _finish(cks)


@pytest.mark.parametrize("shape", BMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bmm_rim_point(shape):
    cks = [_bmm_case(shape, "softmax", lincomb, "rim point", rim=True) for lincomb in (False, True)]
    _report(f"bmm rim point {shape}", cks)
    _finish(cks)


def test_bmm_batch_dimensions_and_an_operand_without_them():
    """Leading batch dimensions (2, 3) on both operands; then xs without them (shared points) and weights without them: the operand
    is expanded on the host and autograd sums its gradient over the batch."""
    g = torch.Generator().manual_seed(23)
    xs = _ball_rows(g, 6 * 7, 5, edge=False).reshape(2, 3, 7, 5)
    w = torch.softmax(torch.randn(2, 3, 4, 7, generator=g), dim=-1)
    go = torch.randn(2, 3, 4, 5, generator=g)
    cks = []
    for tag, x_, w_ in (("both", xs, w), ("xs shared", xs[0, 0], w), ("weights shared", xs, w[0, 0])):
        res = _bmm_refs(None, x_, w_, go, True)
        out, gx, gw = _bmm_run(x_, w_, go, True)
        assert out.shape == (2, 3, 4, 5) and gx.shape == x_.shape and gw.shape == w_.shape
        ck = Ck("bmm batch dims, " + tag)
        for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_w", gw, "gw")):
            ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
        cks.append(ck)
    _report("bmm batch dims", cks)
    _finish(cks)


# ================================================================================================ reduce form
def _red_data(M, R, D, wk, rim=False, seed=0):
    g = torch.Generator().manual_seed(1000003 * M + 1009 * R + D + seed)
    xs = _ball_rows(g, M * R, D, edge=False)
    if rim:
        xs = _rim(xs, g)
    xs = xs.reshape(M, R, D)
    u = torch.rand(M, R, generator=g)
    w = {None: None, "scalar": torch.tensor(1.4 / M), "scalarneg": torch.tensor(-1.4 / M), "pos": (0.1 + 0.9 * u) * (2.0 / M),
         "signed": (2 * u - 1) * (2.0 / M)}[wk]
    return xs, w, torch.randn(R, D, generator=g)


def _red_refs(xs, w, go, flags):
    """out, grad_xs, grad_w of the restatement in fp64 and fp32; for a single weight also ``summands``: the gradient of the weight
    expanded to (M, R)."""
    res = {}
    for dt in (F64, F32):
        x = _leaf(xs, dt)
        ww = None if w is None else _leaf(w, dt)
        o = weighted_midpoint_ref(x, ww, reducedim=[0], **flags)
        gs = torch.autograd.grad(o, [x] + ([] if w is None else [ww]), go.to(dt))
        res[dt] = dict(out=o.detach(), gx=gs[0], gw=None if w is None else gs[1])
        if w is not None and w.numel() == 1 and xs.shape[0] * xs.shape[1] > 1:
            we = _leaf(w.expand(xs.shape[:2]), dt)
            res[dt]["summands"] = torch.autograd.grad(weighted_midpoint_ref(_leaf(xs, dt), we, reducedim=[0], **flags), we, go.to(dt))[0]
    return res


def _red_run(xs, w, go, flags, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd = mk(xs).requires_grad_(True)
    wd = None if w is None else (mk(w) if w.numel() > 1 else w.cuda()).requires_grad_(True)
    out = _gmath().weighted_midpoint(xd, -1.0, weights=wd, reducedim=[0], **flags)
    out.backward(go.cuda())
    return out.detach(), xd.grad, None if w is None else wd.grad


def _red_check(ck, res, out, gx, gw, rows):
    r64, r32 = res[F64], res[F32]
    for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx")):
        assert bool(torch.isfinite(t).all()), (ck.case, name)
        ck.cmp(name, t.cpu(), r64[k], r32[k])
    if gw is None:
        return
    assert bool(torch.isfinite(gw).all()), (ck.case, "grad_w")
    if "summands" in r64:
        ck.red("grad_w (single weight)", gw.cpu().reshape(()), r64["gw"].reshape(()), r64["summands"].abs().sum(), rows,
               sc.grad_allowance(r64["summands"], r32["summands"]))
    else:
        ck.cmp("grad_w", gw.cpu(), r64["gw"], r32["gw"])


def _red_case(shape, wk, flags, tag, rim=False):
    xs, w, go = _red_data(*shape, wk, rim=rim)
    ck = Ck(f"reduce {shape} weights={wk} {flags} {tag}")
    _red_check(ck, _red_refs(xs, w, go, flags), *_red_run(xs, w, go, flags), shape[0] * shape[1])
    return ck


@pytest.mark.parametrize("shape", RED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_forward_and_backward(shape):
    cks = [_red_case(shape, wk, flags, "") for wk, flags in RED_CONFIGS]
    _report(f"reduce {shape}", cks)
    _finish(cks)


@pytest.mark.parametrize("shape", RED_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_reduce_rim_point(shape):
    cks = [_red_case(shape, "pos", flags, "rim point", rim=True) for flags in ({}, dict(lincomb=True))]
    _report(f"reduce rim point {shape}", cks)
    _finish(cks)


@pytest.mark.parametrize("reducedim,wshape,keepdim", [([1], (9, 1), False), ([0, 2], (5, 9, 4), False), ([0, 2], (5, 9, 4), True), (None, (4,), False),
                                                      ([-2], None, True)])
def test_reduce_over_dimensions_that_do_not_lead(reducedim, wshape, keepdim):
    g = torch.Generator().manual_seed(5947)
    xs = _ball_rows(g, 5 * 9 * 4, 7, edge=False).reshape(5, 9, 4, 7)
    w = None if wshape is None else (2 * torch.rand(wshape, generator=g) - 1) * 0.2
    res = {}
    for dt in (F64, F32):
        x, ww = _leaf(xs, dt), None if w is None else _leaf(w, dt)
        o = weighted_midpoint_ref(x, ww, reducedim=reducedim, keepdim=keepdim, lincomb=True, posweight=True)
        if "go" not in res:
            res["go"] = torch.randn(o.shape, generator=g)
        gs = torch.autograd.grad(o, [x] + ([] if w is None else [ww]), res["go"].to(dt))
        res[dt] = dict(out=o.detach(), gx=gs[0], gw=None if w is None else gs[1])
    xd = xs.cuda().requires_grad_(True)
    wd = None if w is None else w.cuda().requires_grad_(True)
    out = _gmath().weighted_midpoint(xd, -1.0, weights=wd, reducedim=reducedim, keepdim=keepdim, lincomb=True, posweight=True)
    assert out.shape == res[F64]["out"].shape
    out.backward(res["go"].cuda())
    ck = Ck(f"reduce (5,9,4,7) reducedim={reducedim} weights {wshape} keepdim={keepdim}")
    ck.cmp("out", out.detach().cpu(), res[F64]["out"], res[F32]["out"])
    ck.cmp("grad_x", xd.grad.cpu(), res[F64]["gx"], res[F32]["gx"])
    if w is not None:
        ck.cmp("grad_w", wd.grad.cpu(), res[F64]["gw"], res[F32]["gw"])
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ mobius_scalar_mul
def _smul_refs(r, x, go):
    res = {}
    for dt in (F64, F32):
        rr, xx = _leaf(r, dt), _leaf(x, dt)
        o = mobius_scalar_mul_ref(rr, xx)
        gr, gx = torch.autograd.grad(o, [rr, xx], go.to(dt))
        res[dt] = dict(out=o.detach(), gr=gr, gx=gx)
        if r.numel() == 1 and x.shape[0] > 1:
            re = _leaf(r.reshape(1, 1).expand(x.shape[0], 1), dt)
            res[dt]["summands"] = torch.autograd.grad(mobius_scalar_mul_ref(re, _leaf(x, dt)), re, go.to(dt))[0]
    return res


def _smul_run(r, x, go, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    rd, xd = r.cuda().requires_grad_(True), mk(x).requires_grad_(True)
    out = _gmath().mobius_scalar_mul(rd, xd, k=-1.0)
    out.backward(go.cuda())
    return out.detach(), rd.grad, xd.grad


def _zero_rows(x):
    return (x == 0).all(dim=1)


@pytest.mark.parametrize("rows,D", [(39, 100), (17, 256), (1, 1), (5, 63)])
@pytest.mark.parametrize("rkind", ["rows", "scalar", "zero", "negative", "large"])
def test_scalar_mul_forward_and_backward(rows, D, rkind):
    """r per row in [-1.5, 2.5]; one r = 1.7, 0, -2.3 and 40 (tanh saturates: the clamp at 15 holds r artanh |x| and nothing flows).
    grad_x of an all-zero row is g tanh(r artanh(1e-15)) / 1e-15, which is r g to thirty digits.  The restatement's artanh is the
    reference's difference of two logarithms: at 1e-15 that is 0 in fp32 and 1.055e-15 in fp64 (1 + 1e-15 and 1 - 1e-15 rounded to
    doubles), so its gradient there is 0 and 1.055 r g, and err32 of a tensor with such a row would allow anything.  The kernels
    take artanh from log1p.  The zero rows of grad_x are therefore left out of the comparison with the restatement and held to r g
    itself, under the same rule with no fp32 error to draw on (its floor F alone)."""
    g = torch.Generator().manual_seed(100 * rows + D)
    x = _ball_rows(g, rows, D, edge=False)
    r = {"rows": torch.rand(rows, 1, generator=g) * 4 - 1.5, "scalar": torch.tensor(1.7), "zero": torch.tensor(0.0), "negative": torch.tensor(-2.3),
         "large": torch.tensor(40.0)}[rkind]
    go = torch.randn(rows, D, generator=g)
    res = _smul_refs(r, x, go)
    out, gr, gx = _smul_run(r, x, go)
    ck = Ck(f"scalar_mul ({rows},{D}) r {rkind}")
    r64, r32 = res[F64], res[F32]
    ck.cmp("out", out.cpu(), r64["out"], r32["out"])
    z = _zero_rows(x)
    live = (~z).numpy()[:, None] & np.ones((rows, D), dtype=bool)
    ck.cmp("grad_x", gx.cpu(), r64["gx"], r32["gx"], mask=live)
    if bool(z.any()):
        exact = (r.double().reshape(-1, 1).expand(rows, 1) * go.double())[z]
        ck.cmp("grad_x (zero rows, against r g)", gx.cpu()[z], exact, exact)
    if "summands" in r64:
        ck.red("grad_r (single r)", gr.cpu().reshape(()), r64["gr"].reshape(()), r64["summands"].abs().sum(), rows,
               sc.grad_allowance(r64["summands"], r32["summands"]))
    else:
        ck.cmp("grad_r", gr.cpu(), r64["gr"], r32["gr"])
    for t in (out, gr, gx):
        assert bool(torch.isfinite(t).all())
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ the reference's recorded cases
def test_recorded_cases_through_the_public_functions():
    from test_weighted_midpoint_host import BMM_KINDS, REDUCE_CASES, SMUL_ZERO_ROW, bmm_name, load_fixture
    gm = _gmath()
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    cks = []
    for kind in BMM_KINDS:
        for lincomb in (False, True):
            xs, w, go = fx["bmm_xs"], fx[f"bmm_w_{kind}"], fx["bmm_grad_output"]
            res = _bmm_refs(None, xs, w, go, lincomb)
            out, gx, gw = _bmm_run(xs, w, go, lincomb)
            ck = Ck("recorded " + bmm_name(kind, lincomb))
            for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_w", gw, "gw")):
                ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
            if kind == "zerow":
                assert bool((out[1, 3] == 0).all()) and bool(torch.isfinite(gw).all()) and bool(torch.isfinite(gx).all())
            cks.append(ck)
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in REDUCE_CASES.items():
        xs, w = fx["red_xs"], None if wk is None else fx[f"red_w_{wk}"]
        go = fx["red_grad_output_all" if reducedim is None else "red_grad_output_r0"]
        flags = dict(keepdim=keepdim, lincomb=lincomb, posweight=posweight, coadd=coadd)
        res = {}
        for dt in (F64, F32):
            x, ww = _leaf(xs, dt), None if w is None else _leaf(w, dt)
            o = weighted_midpoint_ref(x, ww, reducedim=reducedim, **flags)
            gs = torch.autograd.grad(o, [x] + ([] if w is None else [ww]), go.to(dt).reshape(o.shape))
            res[dt] = dict(out=o.detach(), gx=gs[0], gw=None if w is None else gs[1])
        xd = xs.cuda().requires_grad_(True)
        wd = None if w is None else w.cuda().requires_grad_(True)
        out = gm.weighted_midpoint(xd, -1.0, weights=wd, reducedim=reducedim, **flags)
        assert tuple(out.shape) == tuple(fx[f"red_{name}.out"].shape)
        out.backward(go.cuda().reshape(out.shape))
        ck = Ck("recorded red_" + name)
        ck.cmp("out", out.detach().cpu(), res[F64]["out"], res[F32]["out"])
        ck.cmp("grad_x", xd.grad.cpu(), res[F64]["gx"], res[F32]["gx"])
        if w is not None and w.numel() > 1:
            ck.cmp("grad_w", wd.grad.cpu(), res[F64]["gw"], res[F32]["gw"])
        elif w is not None:
            terms = _red_refs(xs, w, go, dict(lincomb=lincomb, posweight=posweight, coadd=coadd))
            ck.red("grad_w (single weight)", wd.grad.cpu().reshape(()), res[F64]["gw"].reshape(()), terms[F64]["summands"].abs().sum(), 54,
                   sc.grad_allowance(terms[F64]["summands"], terms[F32]["summands"]))
        cks.append(ck)
    for name in ("smul_rows", "smul_scalar"):
        r, x, go = fx["smul_r_" + name[5:]], fx["smul_x"], fx["smul_grad_output"]
        res = _smul_refs(r, x, go)
        out, gr, gx = _smul_run(r, x, go)
        ck = Ck("recorded " + name)
        ck.cmp("out", out.cpu(), res[F64]["out"], res[F32]["out"])
        live = np.ones((9, 5), dtype=bool)
        live[SMUL_ZERO_ROW] = False
        ck.cmp("grad_x", gx.cpu(), res[F64]["gx"], res[F32]["gx"], mask=live)
        if r.numel() > 1:
            ck.cmp("grad_r", gr.cpu(), res[F64]["gr"], res[F32]["gr"])
        else:
            ck.red("grad_r (single r)", gr.cpu().reshape(()), res[F64]["gr"].reshape(()), res[F64]["summands"].abs().sum(), 9,
                   sc.grad_allowance(res[F64]["summands"], res[F32]["summands"]))
        cks.append(ck)
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ degenerate inputs
def test_all_zero_points_and_an_all_zero_weight_row():
    g = torch.Generator().manual_seed(77)
    cks = []
    xs, w, go = torch.zeros(2, 33, 20), torch.randn(2, 17, 33, generator=g) * 0.1, torch.randn(2, 17, 20, generator=g)
    for lincomb in (False, True):
        res = _bmm_refs(None, xs, w, go, lincomb)
        out, gx, gw = _bmm_run(xs, w, go, lincomb)
        assert bool((out == 0).all()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        ck = Ck(f"bmm, all-zero points, lincomb={lincomb}")
        ck.cmp("grad_x", gx.cpu(), res[F64]["gx"], res[F32]["gx"])
        ck.cmp("grad_w", gw.cpu(), res[F64]["gw"], res[F32]["gw"])
        cks.append(ck)
    xs, w, go = _bmm_data(2, 17, 33, 20, "signed")
    w[1, 5] = 0.0
    for lincomb in (False, True):
        res = _bmm_refs(None, xs, w, go, lincomb)
        out, gx, gw = _bmm_run(xs, w, go, lincomb)
        assert bool((out[1, 5] == 0).all()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
        ck = Ck(f"bmm, an all-zero weight row, lincomb={lincomb}")
        for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_w", gw, "gw")):
            ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
        cks.append(ck)
    xs, w, go = torch.zeros(9, 6, 5), torch.rand(9, 6, generator=g) - 0.5, torch.randn(6, 5, generator=g)
    w[:, 2] = 0.0                                           # and a kept row whose weights are all zero
    for flags in ({}, dict(lincomb=True, posweight=True)):
        out, gx, gw = _red_run(xs, w, go, flags)
        assert bool((out == 0).all())
        ck = Ck(f"reduce, all-zero points, {flags}")
        _red_check(ck, _red_refs(xs, w, go, flags), out, gx, gw, 54)
        cks.append(ck)
    _report("degenerate inputs", cks)
    _finish(cks)


# ================================================================================================ the same bits
def _equal(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def test_operands_at_storage_offset_1_give_the_same_bits():
    xs, w, go = _bmm_data(2, 65, 129, 100, "signed")
    _equal(_bmm_run(xs, w, go, True), _bmm_run(xs, w, go, True, unaligned=True), "bmm")
    xs, w, go = _red_data(33, 17, 63, "signed")
    f = dict(lincomb=True, posweight=True)
    _equal(_red_run(xs, w, go, f), _red_run(xs, w, go, f, unaligned=True), "reduce")
    g = torch.Generator().manual_seed(3)
    x, r, go = _ball_rows(g, 39, 100, edge=False), torch.rand(39, 1, generator=g) * 2, torch.randn(39, 100, generator=g)
    _equal(_smul_run(r, x, go), _smul_run(r, x, go, unaligned=True), "scalar_mul")


def test_inference_has_the_bits_of_the_training_form():
    gm = _gmath()
    xs, w, go = _bmm_data(2, 65, 129, 100, "signed")
    trained = _bmm_run(xs, w, go, True)[0]
    with torch.no_grad():
        assert torch.equal(gm.weighted_midpoint_bmm(xs.cuda(), w.cuda(), -1.0, lincomb=True), trained)
    for shape in ((33, 17, 63), (4099, 1, 20)):
        xs, w, go = _red_data(*shape, "signed")
        trained = _red_run(xs, w, go, dict(lincomb=True))[0]
        with torch.no_grad():
            assert torch.equal(gm.weighted_midpoint(xs.cuda(), -1.0, weights=w.cuda(), reducedim=[0], lincomb=True), trained)


def test_each_null_gradient_combination_has_the_bits_of_the_full_run():
    c = _C()
    batch, N, M, D = 2, 17, 33, 20
    xs, w, go = (t.cuda() for t in _bmm_data(batch, N, M, D, "signed"))
    out, saved = torch.empty(batch, N, D, device="cuda"), torch.empty(batch, N, D + 2, device="cuda")
    c.check(c.lib.hypad_weighted_midpoint_bmm_fwd(c.ptr(xs), c.ptr(w), c.ptr(out), c.ptr(saved), batch, N, M, D, LINCOMB, c.stream()))
    need = c.lib.hypad_weighted_midpoint_bmm_workspace_bytes(batch, N, M, D)
    full = None
    for sel in (3, 2, 1, 0):
        ws = torch.full((need // 4,), NAN, device="cuda")
        outs = [torch.full(tuple(t.shape), NAN, device="cuda") if sel >> i & 1 else None for i, t in enumerate((xs, w))]
        c.check(c.lib.hypad_weighted_midpoint_bmm_bwd(c.ptr(xs), c.ptr(w), c.ptr(saved), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), c.ptr(ws), need,
                                                      batch, N, M, D, LINCOMB, c.stream()), f"bmm_bwd {sel:02b}")
        full = full or outs
        _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"bmm {sel:02b}")
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all())
    M, R, D = 33, 17, 63
    for wk in ("signed", "scalar"):
        xs, w, go = (t.cuda() for t in _red_data(M, R, D, wk))
        out, saved = torch.empty(R, D, device="cuda"), torch.empty(R, D + 2, device="cuda", dtype=F64)
        need = c.lib.hypad_weighted_midpoint_workspace_bytes(M, R, D)
        ws = torch.full((need // 4,), NAN, device="cuda")
        c.check(c.lib.hypad_weighted_midpoint_fwd(c.ptr(xs), c.ptr(w), w.numel(), c.ptr(out), c.ptr(saved), c.ptr(ws), need, M, R, D, LINCOMB, c.stream()))
        full = None
        for sel in (3, 2, 1, 0):
            ws = torch.full((need // 4,), NAN, device="cuda")
            outs = [torch.full(tuple(t.shape), NAN, device="cuda") if sel >> i & 1 else None for i, t in enumerate((xs, w.reshape(-1)))]
            c.check(c.lib.hypad_weighted_midpoint_bwd(c.ptr(xs), c.ptr(w), w.numel(), c.ptr(saved), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), c.ptr(ws),
                                                      need, M, R, D, LINCOMB, c.stream()), f"reduce_bwd {sel:02b}")
            full = full or outs
            _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"reduce {wk} {sel:02b}")
        assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all())
    g = torch.Generator().manual_seed(5)
    x, r, go = (t.cuda() for t in (_ball_rows(g, 39, 100, edge=False), torch.rand(39, generator=g) * 2, torch.randn(39, 100, generator=g)))
    full = None
    for sel in (3, 2, 1, 0):
        outs = [torch.full(s, NAN, device="cuda") if sel >> i & 1 else None for i, s in enumerate(((39,), (39, 100)))]
        c.check(c.lib.hypad_mobius_scalar_mul_bwd(c.ptr(r), c.ptr(x), c.ptr(go), c.ptr(outs[0]), c.ptr(outs[1]), 39, 100, 39, c.stream()))
        full = full or outs
        _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"scalar_mul {sel:02b}")
    assert bool(torch.isfinite(full[0]).all()) and bool(torch.isfinite(full[1]).all())


def test_two_backward_runs_give_the_same_bits():
    for run, data, extra in ((_red_run, _red_data(4099, 1, 20, "signed"), dict(lincomb=True)), (_bmm_run, _bmm_data(1, 17, 4099, 20, "signed"), True)):
        got = []
        for _ in range(2):
            got.append(run(*data, extra))
            torch.full((4099 * 20 * 7,), NAN, device="cuda")   # (another history of the allocator's blocks between the runs)
        _equal(got[0], got[1], run.__name__)
    xs, w, go = _bmm_data(1, 17, 4099, 20, "signed")
    res = _bmm_refs(None, xs, w, go, True)
    ck = Ck("bmm (1,17,4099,20): 65 chunks")
    for name, t, k in zip(("out", "grad_x", "grad_w"), _bmm_run(xs, w, go, True), ("out", "gx", "gw")):
        ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
    _finish([ck])


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    batch, N, M, D = 2, 17, 33, 20
    xs, w, go = _bmm_data(batch, N, M, D, "signed")
    res = _bmm_refs(None, xs, w, go, True)
    xd, wd, god = xs.cuda(), w.cuda(), go.cuda()
    bufs = [_guarded(s, o) for s, o in (((batch, N, D), 3), ((batch, N, D + 2), 5), ((batch, M, D), 1), ((batch, N, M), 2))]
    (_, out), (_, saved), (_, gx), (_, gw) = bufs
    c.check(c.lib.hypad_weighted_midpoint_bmm_fwd(c.ptr(xd), c.ptr(wd), c.ptr(out), c.ptr(saved), batch, N, M, D, LINCOMB, c.stream()))
    need = c.lib.hypad_weighted_midpoint_bmm_workspace_bytes(batch, N, M, D)
    wbuf, ws = _guarded((need // 4,), 4)
    c.check(c.lib.hypad_weighted_midpoint_bmm_bwd(c.ptr(xd), c.ptr(wd), c.ptr(saved), c.ptr(god), c.ptr(gx), c.ptr(gw), c.ptr(ws), need, batch, N, M, D,
                                                  LINCOMB, c.stream()))
    torch.cuda.synchronize()
    for (buf, v), off in zip(bufs + [(wbuf, ws)], (3, 5, 1, 2, 4)):
        assert _guards_intact(buf, off)
    ck = Ck("guarded bmm (2,17,33,20)")
    for name, t, k in (("out", out, "out"), ("grad_x", gx, "gx"), ("grad_w", gw, "gw")):
        assert bool(torch.isfinite(t).all())
        ck.cmp(name, t.cpu(), res[F64][k], res[F32][k])
    for M, R, D, wk in ((33, 17, 63, "signed"), (4099, 1, 20, "scalar")):
        xs, w, go = _red_data(M, R, D, wk)
        rres = _red_refs(xs, w, go, dict(lincomb=True))
        xd, wd, god = xs.cuda(), w.cuda(), go.cuda()
        bufs = [_guarded(s, o) for s, o in (((R, D), 3), ((R, 2 * (D + 2)), 6), ((M, R, D), 1), ((w.numel(),), 2))]     # (saved: fp64, two floats each)
        (_, out), (_, saved), (_, gx), (_, gw) = bufs
        need = c.lib.hypad_weighted_midpoint_workspace_bytes(M, R, D)
        wbuf, ws = _guarded((need // 4,), 16)
        c.check(c.lib.hypad_weighted_midpoint_fwd(c.ptr(xd), c.ptr(wd), w.numel(), c.ptr(out), c.ptr(saved), c.ptr(ws), need, M, R, D, LINCOMB, c.stream()))
        c.check(c.lib.hypad_weighted_midpoint_bwd(c.ptr(xd), c.ptr(wd), w.numel(), c.ptr(saved), c.ptr(god), c.ptr(gx), c.ptr(gw), c.ptr(ws), need, M, R, D,
                                                  LINCOMB, c.stream()))
        torch.cuda.synchronize()
        for (buf, v), off in zip(bufs + [(wbuf, ws)], (3, 6, 1, 2, 16)):
            assert _guards_intact(buf, off)
        _red_check(ck, rres, out, gx, gw.reshape(w.shape), M * R)
    g = torch.Generator().manual_seed(9)
    x, r, go = _ball_rows(g, 17, 256, edge=False), torch.rand(17, 1, generator=g) * 2, torch.randn(17, 256, generator=g)
    sres = _smul_refs(r, x, go)
    bufs = [_guarded(s, o) for s, o in (((17, 256), 3), ((17,), 5), ((17, 256), 1))]
    (_, out), (_, gr), (_, gx) = bufs
    xd, rd, god = x.cuda(), r.cuda(), go.cuda()
    c.check(c.lib.hypad_mobius_scalar_mul_fwd(c.ptr(rd), c.ptr(xd), c.ptr(out), 17, 256, 17, c.stream()))
    c.check(c.lib.hypad_mobius_scalar_mul_bwd(c.ptr(rd), c.ptr(xd), c.ptr(god), c.ptr(gr), c.ptr(gx), 17, 256, 17, c.stream()))
    torch.cuda.synchronize()
    for (buf, v), off in zip(bufs, (3, 5, 1)):
        assert _guards_intact(buf, off)
    ck.cmp("scalar_mul out", out.cpu(), sres[F64]["out"], sres[F32]["out"])
    ck.cmp("scalar_mul grad_r", gr.cpu().reshape(17, 1), sres[F64]["gr"], sres[F32]["gr"])
    live = (~_zero_rows(x)).numpy()[:, None] & np.ones((17, 256), dtype=bool)
    ck.cmp("scalar_mul grad_x", gx.cpu(), sres[F64]["gx"], sres[F32]["gx"], mask=live)
    _finish([ck])


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    batch, N, M = 2, 4, 6
    for D in (257, 8):
        xs, w, go = (torch.zeros(s, device="cuda") for s in ((batch, M, D), (batch, N, M), (batch, N, D)))
        # (saved: room for the bmm form's (batch, N, D + 2) floats and for the reduce form's (R = M, D + 2) doubles)
        out, saved, gx, gw = (torch.full(s, SENTINEL, device="cuda") for s in ((batch, N, D), (batch * M, 2 * (D + 2)), (batch, M, D), (batch, N, M)))
        need = max(L.hypad_weighted_midpoint_bmm_workspace_bytes(batch, N, M, min(D, 256)), 8)
        ws = torch.full((need // 4,), SENTINEL, device="cuda")
        fwd = lambda x=xs, ww=w, o=out, b=batch, n=N, m=M, d=D, f=0: L.hypad_weighted_midpoint_bmm_fwd(c.ptr(x), c.ptr(ww), c.ptr(o), c.ptr(saved), b, n, m, d,
                                                                                                       f, c.stream())
        bwd = lambda x=xs, sv=saved, nb=need, b=batch, n=N, m=M, d=D, f=0: L.hypad_weighted_midpoint_bmm_bwd(
            c.ptr(x), c.ptr(w), c.ptr(sv), c.ptr(go), c.ptr(gx), c.ptr(gw), c.ptr(ws), nb, b, n, m, d, f, c.stream())
        # reduce form on the same buffers: xs as (M' = batch, R = M, D), weights (batch, M) from w's storage
        rneed = max(L.hypad_weighted_midpoint_workspace_bytes(batch, M, min(D, 256)), 8)
        rws = torch.full((rneed // 4,), SENTINEL, device="cuda")
        rfwd = lambda x=xs, ww=w, wc=batch * M, o=out, m=batch, r=M, d=D, f=0: L.hypad_weighted_midpoint_fwd(c.ptr(x), c.ptr(ww), wc, c.ptr(o), c.ptr(saved),
                                                                                                             c.ptr(rws), rneed, m, r, d, f, c.stream())
        rbwd = lambda x=xs, ww=w, wc=batch * M, nb=rneed, m=batch, r=M, d=D, f=0, g=gw: L.hypad_weighted_midpoint_bwd(
            c.ptr(x), c.ptr(ww), wc, c.ptr(saved), c.ptr(go), c.ptr(gx), c.ptr(g), c.ptr(rws), nb, m, r, d, f, c.stream())
        # scalar mul over the batch * M rows of xs, r = w[0]; out and grad_x into gx (batch * M rows), grad_r into gw, xs as grad_out
        sfwd = lambda r=w, x=xs, n=batch * M, d=D, rr=1: L.hypad_mobius_scalar_mul_fwd(c.ptr(r), c.ptr(x), c.ptr(gx), n, d, rr, c.stream())
        sbwd = lambda r=w, x=xs, n=batch * M, d=D, rr=1: L.hypad_mobius_scalar_mul_bwd(c.ptr(r), c.ptr(x), c.ptr(xs), c.ptr(gw), c.ptr(gx), n, d, rr, c.stream())
        if D == 257:
            for call in (fwd, bwd, rfwd, rbwd, sfwd, sbwd):
                assert call() == HYPAD_EUNSUPPORTED
        else:
            assert fwd(x=None) == fwd(ww=None) == fwd(o=None) == bwd(x=None) == bwd(sv=None) == HYPAD_EINVAL
            assert fwd(b=0) == fwd(n=-1) == fwd(m=0) == fwd(d=0) == fwd(f=2) == fwd(f=8) == HYPAD_EINVAL
            assert bwd(b=-1) == bwd(m=0) == bwd(d=-2) == bwd(f=4) == HYPAD_EINVAL
            assert bwd(nb=need - 4) == HYPAD_EWORKSPACE
            assert rfwd(x=None) == rfwd(o=None) == rfwd(m=0) == rfwd(r=-1) == rfwd(d=0) == rfwd(f=8) == rfwd(wc=5) == rfwd(ww=None) == HYPAD_EINVAL
            assert rbwd(x=None) == rbwd(m=0) == rbwd(f=16) == rbwd(wc=3) == rbwd(ww=None, wc=0) == HYPAD_EINVAL     # (a gradient for weights that are not there)
            assert rbwd(nb=rneed - 4) == HYPAD_EWORKSPACE
            assert sfwd(r=None) == sfwd(x=None) == sfwd(n=-1) == sfwd(d=0) == sfwd(rr=5) == sbwd(r=None) == sbwd(rr=7) == HYPAD_EINVAL
        torch.cuda.synchronize()
        for t in (out, saved, gx, gw, ws, rws):
            assert bool((t == SENTINEL).all())              # nothing ran
    assert fwd() == 0 and bwd() == 0 and rfwd() == 0 and rbwd() == 0 and sfwd() == 0 and sbwd() == 0
    # the sliced forward needs its workspace
    xs, out = torch.zeros(4099, 1, 20, device="cuda"), torch.full((1, 20), SENTINEL, device="cuda")
    need = L.hypad_weighted_midpoint_workspace_bytes(4099, 1, 20)
    ws = torch.full((need // 4,), SENTINEL, device="cuda")
    assert L.hypad_weighted_midpoint_fwd(c.ptr(xs), None, 0, c.ptr(out), None, c.ptr(ws), need - 4, 4099, 1, 20, 0, c.stream()) == HYPAD_EWORKSPACE
    assert L.hypad_weighted_midpoint_fwd(c.ptr(xs), None, 0, c.ptr(out), None, None, 0, 4099, 1, 20, 0, c.stream()) == HYPAD_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ws == SENTINEL).all())
    with pytest.raises(NotImplementedError, match="supported"):
        _gmath().weighted_midpoint_bmm(torch.zeros(2, 4, 257, device="cuda"), torch.zeros(2, 3, 4, device="cuda"), -1.0)


def test_no_output_rows_leave_zero_gradients():
    c = _C()
    xs, w, go = torch.zeros(2, 6, 8, device="cuda"), torch.zeros(2, 0, 6, device="cuda"), torch.zeros(2, 0, 8, device="cuda")
    gx = torch.full((2, 6, 8), NAN, device="cuda")
    assert c.lib.hypad_weighted_midpoint_bmm_fwd(c.ptr(xs), c.ptr(w), None, None, 2, 0, 6, 8, 0, c.stream()) == 0
    assert c.lib.hypad_weighted_midpoint_bmm_bwd(c.ptr(xs), c.ptr(w), None, None, c.ptr(gx), None, None, 0, 2, 0, 6, 8, 0, c.stream()) == 0
    assert bool((gx == 0).all())
    gw = torch.full((1,), NAN, device="cuda")
    one = torch.ones(1, device="cuda")
    assert c.lib.hypad_weighted_midpoint_fwd(c.ptr(xs), c.ptr(one), 1, None, None, None, 0, 6, 0, 8, 0, c.stream()) == 0
    assert c.lib.hypad_weighted_midpoint_bwd(c.ptr(xs), c.ptr(one), 1, None, None, None, c.ptr(gw), None, 0, 6, 0, 8, 0, c.stream()) == 0
    assert float(gw) == 0.0


# ================================================================================================ side stream, captured graph
def _stream_cases():
    xs, w, go = _bmm_data(2, 65, 129, 100, "signed")
    rx, rw, rgo = _red_data(100, 64, 100, "signed")
    gm = _gmath()
    return [("bmm", (xs, w, go), lambda a, b: gm.weighted_midpoint_bmm(a, b, -1.0, lincomb=True)),
            ("reduce", (rx, rw, rgo), lambda a, b: gm.weighted_midpoint(a, -1.0, weights=b, reducedim=[0], lincomb=True, posweight=True))]


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


# ================================================================================================ stacks
def test_gru_pooled_over_its_steps_and_read_out_takes_an_sgd_step():
    """mobius_gru_loop (T = 3) -> weighted_midpoint over the steps -> MobiusDist2Hyperplane -> cross-entropy -> one SGD step: a sequence
    classifier that stays on the ball.  The restatement: tests/mobius_gru_ref.py, midpoint_ref.py, dist2plane_ref.py."""
    from dist2plane_ref import dist2plane_parts
    from hypad_amd.hyperspace import hyrnn_nets
    import mobius_gru_ref as gr
    T, rows, I, H, N = 3, 9, 7, 20, 5
    g = torch.Generator().manual_seed(3972005)
    x = _ball_rows(g, T * rows, I, edge=False, radius=0.8).reshape(T, rows, I)
    h0 = _ball_rows(g, rows, H, edge=False, radius=0.5)
    w_ih = (torch.rand(3 * H, I, generator=g) * 2 - 1) / H ** 0.5
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) / H ** 0.5
    bias = _ball_rows(g, 3, H, edge=False, zero_row=False, radius=0.5)
    point, tangent = _ball_rows(g, N, H, radius=0.8, edge=False, zero_row=False), torch.randn(N, H, generator=g)
    scale, target = 0.3 * torch.randn(N, generator=g), torch.randint(0, N, (rows,), generator=g)
    wsteps = torch.tensor([0.2, 0.3, 0.5])
    names = ("x", "h0", "w_ih", "w_hh", "bias", "point", "tangent", "scale", "wsteps")
    res = {}
    for dt in (F64, F32):
        p = {n: _leaf(t, dt) for n, t in zip(names, (x, h0, w_ih, w_hh, bias, point, tangent, scale, wsteps))}
        outs = gr.gru_loop_ref(p["x"], p["h0"], p["w_ih"], p["w_hh"], p["bias"])[0]
        pooled = weighted_midpoint_ref(outs, p["wsteps"].reshape(T, 1), reducedim=[0])
        logits, _ = dist2plane_parts(pooled, p["point"], p["tangent"], True, False, p["scale"])
        loss = torch.nn.functional.cross_entropy(logits, target)
        gs = torch.autograd.grad(loss, [p[n] for n in names])
        res[dt] = dict(logits=logits.detach(), loss=loss.detach(), pooled=pooled.detach(), **{"g_" + n: v for n, v in zip(names, gs)})
    head = hyrnn_nets.MobiusDist2Hyperplane(H, N)
    with torch.no_grad():
        head.point.copy_(point), head.tangent.copy_(tangent), head.scale.copy_(scale)
    head = head.cuda()
    d = {n: t.cuda().requires_grad_(True) for n, t in zip(names[:5] + names[8:], (x, h0, w_ih, w_hh, bias, wsteps))}
    params = [d["w_ih"], d["w_hh"], d["bias"], d["wsteps"]] + list(head.parameters())
    before = [q.detach().clone() for q in params]
    opt = torch.optim.SGD(params, lr=0.1)
    outs = hyrnn_nets.mobius_gru_loop(d["x"], d["h0"], d["w_ih"], d["w_hh"], d["bias"], k=-1.0, hyperbolic_input=True, hyperbolic_hidden_state0=True)[0]
    pooled = _gmath().weighted_midpoint(outs, -1.0, weights=d["wsteps"].reshape(T, 1), reducedim=[0])
    logits = head(pooled)
    loss = torch.nn.functional.cross_entropy(logits, target.cuda())
    loss.backward()
    ck = Ck("GRU -> midpoint over steps -> dist2plane")
    r64, r32 = res[F64], res[F32]
    for name, t in (("pooled", pooled.detach()), ("logits", logits.detach()), ("loss", loss.detach()), ("g_x", d["x"].grad), ("g_h0", d["h0"].grad),
                    ("g_w_ih", d["w_ih"].grad), ("g_w_hh", d["w_hh"].grad), ("g_bias", d["bias"].grad), ("g_wsteps", d["wsteps"].grad),
                    ("g_point", head.point.grad), ("g_tangent", head.tangent.grad), ("g_scale", head.scale.grad)):
        ck.cmp(name, t.cpu(), r64[name], r32[name], steps=T)
    opt.step()
    for q, q0 in zip(params, before):
        assert not torch.equal(q, q0) and torch.equal(q.detach(), torch.add(q0, q.grad, alpha=-0.1))
    _report(ck.case, [ck])
    _finish([ck])


def test_one_head_attention_block():
    """torch softmax of Euclidean scores -> weighted_midpoint_bmm -> MobiusLinear (ball input), forward and every gradient."""
    from hypad_amd.hyperspace import hyrnn_nets
    from test_mobius_modes_host import mobius_linear_ref
    batch, T, D, O = 3, 17, 20, 11
    g = torch.Generator().manual_seed(31720)
    v = _ball_rows(g, batch * T, D, edge=False, radius=0.9).reshape(batch, T, D)
    q, kk = torch.randn(batch, T, D, generator=g), torch.randn(batch, T, D, generator=g)
    w = torch.randn(O, D, generator=g) / D ** 0.5
    b = _ball_rows(g, 1, O, radius=0.5)[0]
    go = torch.randn(batch, T, O, generator=g)
    res = {}
    for dt in (F64, F32):
        vv, qq, k2, ww = (_leaf(t, dt) for t in (v, q, kk, w))
        br = b.to(dt).unsqueeze(0).expand(batch * T, -1).clone().requires_grad_(True)
        att = torch.softmax(qq @ k2.transpose(-1, -2) / D ** 0.5, dim=-1)
        mid = weighted_midpoint_bmm_ref(vv, att)
        o, mx = mobius_linear_ref(mid.reshape(batch * T, D), ww, br, True, True, None)
        gs = torch.autograd.grad(o, [vv, qq, k2, ww, br, mx], go.to(dt).reshape(batch * T, O))
        res[dt] = dict(out=o.detach().reshape(batch, T, O), mid=mid.detach(), g_v=gs[0], g_q=gs[1], g_k=gs[2], g_w=gs[3], gbr=gs[4], gmx=gs[5])
    lin = hyrnn_nets.MobiusLinear(D, O, fp64_hyper=False)
    with torch.no_grad():
        lin.weight.copy_(w), lin.bias.copy_(b)
    lin = lin.cuda()
    vd, qd, kd = (t.cuda().requires_grad_(True) for t in (v, q, kk))
    att = torch.softmax(qd @ kd.transpose(-1, -2) / D ** 0.5, dim=-1)
    mid = _gmath().weighted_midpoint_bmm(vd, att, -1.0)
    out = lin(mid)
    out.backward(go.cuda())
    ck = Ck("softmax -> weighted_midpoint_bmm -> MobiusLinear")
    r64, r32 = res[F64], res[F32]
    for name, t in (("mid", mid.detach()), ("out", out.detach()), ("g_v", vd.grad), ("g_q", qd.grad), ("g_k", kd.grad)):
        ck.cmp(name, t.cpu(), r64[name], r32[name])
    # the layer's sums over rows, as tests/test_gpu_mobius_modes.py holds them: grad_weight = g_mx^T mid, grad_bias = the per-row gradients' sum
    m64 = r64["mid"].reshape(batch * T, D)
    ck.red("g_w", lin.weight.grad.cpu(), r64["g_w"], r64["gmx"].abs().t() @ m64.abs(), batch * T,
           sc.grad_allowance(r64["gmx"], r32["gmx"]) * float(m64.abs().max()) + sc.grad_allowance(r64["mid"], r32["mid"]) * float(r64["gmx"].abs().max()))
    ck.red("g_b", lin.bias.grad.cpu(), r64["gbr"].sum(0), r64["gbr"].abs().sum(0), batch * T, sc.grad_allowance(r64["gbr"], r32["gbr"]))
    _report(ck.case, [ck])
    _finish([ck])
