"""The Moebius GRU on the GPU (hypad_mobius_gru_*, hypad_mobius_pointwise_mul_*; hyperspace/hyrnn_nets.mobius_gru_cell / mobius_gru_loop
and gmath.mobius_pointwise_mul run them) against the plain-torch restatement of tests/mobius_gru_ref.py -- which
tests/test_mobius_gru_host.py pins to the reference's own outputs -- run in fp64 and fp32 on the CPU, under the two rules of
tests/sweep_common.py, unchanged: per-row quantities (outs, h_last, grad_x, grad_h0) under ``Ck.cmp(..., steps=T)``, sums over
T * rows rows (grad_w_ih, grad_w_hh, grad_bias) under ``Ck.red``.  No tolerance of its own.

The reductions.  The backward adds up, over every (step, row),
    grad_w_ih = sum G_mx^T x_t      grad_w_hh = [sum G_mhr^T h_{t-1} ; sum G_mrh^T rh_t ; sum G_mhz^T h_{t-1}]      grad_bias = sum g_b
where G_* are the gradients of the six products and g_b the per-row bias gradients.  ``abs_terms`` is the fp64 sum of the absolute values
of exactly these summands (the restatement hands out the nodes).  The summand allowance: a summand G * v is off by at most
al(G) * max|v| + max|G| * al(v), with al(.) the per-row rule's own allowance of that node (``sweep_common.grad_allowance``: the fp32
restatement against fp64) -- v is an input (x_t: then al(v) is the rule's floor alone) or a value the recurrence computed (h_{t-1}, rh_t).

The data.  x_t and h0: ``_ball_rows`` (radius <= 0.95, the last row all zero); weights U(+-1/sqrt(H)); the bias on the ball within radius
0.5; grad_outs ~ N(0, 1).  The 1 - 1e-3 rim row of h0 and of x_0 is compared alone (``test_gru_rim_row``): with it in the tensor, err32
of the whole tensor would be that row's.
"""
import pytest
import torch

import sweep_common as sc
from mobius_gru_ref import NONLINS, gru_loop_ref, gru_packed_ref, pointwise_mul_ref
from sweep_common import NAN, SENTINEL, Ck, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EWORKSPACE, HYPAD_EUNSUPPORTED = -1, -2, -3          # include/hypad.h
CODES = {"none": 0, "tanh": 1, "relu": 2}                                 # HYPAD_NONLIN_*
SHAPES = [(1, 1, 1, 1), (3, 5, 7, 2), (17, 33, 63, 3), (16, 64, 64, 4), (39, 100, 100, 5), (33, 129, 65, 2), (17, 51, 256, 2), (18, 256, 256, 2),
          (65, 100, 20, 16)]                                              # (rows, I, H, T)
NONLIN_SHAPES = [(17, 33, 63, 3), (39, 100, 100, 5)]
NODES = ("mx", "mhr", "mhz", "mrh", "bias")


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\nmobius_gru {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")


def _data(g, rows, I, H, T, rim=False):
    x = _ball_rows(g, T * rows, I, edge=False).reshape(T, rows, I).double()
    h0 = _ball_rows(g, rows, H, edge=False).double()
    if rim:
        i = 1 if rows >= 3 else 0
        x[0, i] = torch.randn(I, generator=g, dtype=F64)
        h0[i] = torch.randn(H, generator=g, dtype=F64)
        x[0, i] *= (1 - 1e-3) / float(x[0, i].norm())
        h0[i] *= (1 - 1e-3) / float(h0[i].norm())
    s = 1 / H ** 0.5
    w_ih = (torch.rand(3 * H, I, generator=g) * 2 - 1) * s
    w_hh = (torch.rand(3 * H, H, generator=g) * 2 - 1) * s
    bias = _ball_rows(g, 3, H, radius=0.5, edge=False, zero_row=False)
    return x.float(), h0.float(), w_ih, w_hh, bias, torch.randn(T, rows, H, generator=g)


_REFS = {}


def _refs(key, x, h0, w_ih, w_hh, bias, gos, nonlin="none", hyper=(True, True), batch_sizes=None):
    """fp64 and fp32 restatement of one case: the outputs, the gradients of the operands and, per step, the nodes of the reductions with
    their gradients.  gos: the gradient of outs, or of (outs, h_last).  Computed once per key and shared (never modified)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        xx, hh, wi, wh = (_leaf(t, dt) for t in (x, h0, w_ih, w_hh))
        if batch_sizes is None:
            outs, hl, parts = gru_loop_ref(xx, hh, wi, wh, bias.to(dt), NONLINS[nonlin], *hyper, bias_rows=True)
        else:
            outs, hl, parts = gru_packed_ref(xx, hh, wi, wh, bias.to(dt), batch_sizes, NONLINS[nonlin], *hyper, bias_rows=True)
        nodes = [p[k] for p in parts for k in NODES]
        gs = torch.autograd.grad([outs, hl][:len(gos)], [xx, hh, wi, wh] + nodes, [g.to(dt) for g in gos])
        H = h0.shape[1]
        g = {k: torch.cat([gs[4 + len(NODES) * t + j] for t in range(len(parts))]) for j, k in enumerate(NODES[:4])}
        g["bias"] = torch.cat([gs[4 + len(NODES) * t + 4].permute(1, 0, 2).reshape(-1, 3 * H) for t in range(len(parts))])
        v = {k: torch.cat([p[k].detach() for p in parts]) for k in ("x", "hprev", "rh")}
        res[dt] = dict(outs=outs.detach(), h_last=hl.detach(), gx=gs[0], gh0=gs[1], gwi=gs[2], gwh=gs[3], gb=g["bias"].sum(0).reshape(3, H), g=g, v=v)
    if key is not None:
        _REFS[key] = res
    return res


def _reductions(ck, res, gwi, gwh, gb):
    r64, r32 = res[F64], res[F32]
    g64, v64 = r64["g"], r64["v"]
    tr, H = g64["mx"].shape[0], g64["mhr"].shape[1]
    al_g = {k: sc.grad_allowance(g64[k], r32["g"][k]) for k in NODES}
    al_v = {k: sc.grad_allowance(v64[k], r32["v"][k]) for k in v64}
    summand = lambda gk, vk: al_g[gk] * float(v64[vk].abs().max()) + float(g64[gk].abs().max()) * al_v[vk]
    if gwi is not None:
        ck.red("grad_w_ih", gwi, r64["gwi"], g64["mx"].abs().t() @ v64["x"].abs(), tr, summand("mx", "x"))
    if gwh is not None:
        for b, (gk, vk) in enumerate((("mhr", "hprev"), ("mrh", "rh"), ("mhz", "hprev"))):
            ck.red(f"grad_w_hh[{'rhz'[b]}]", gwh[b * H:(b + 1) * H], r64["gwh"][b * H:(b + 1) * H], g64[gk].abs().t() @ v64[vk].abs(), tr, summand(gk, vk))
    if gb is not None:
        ck.red("grad_bias", gb.reshape(-1), g64["bias"].sum(0), g64["bias"].abs().sum(0), tr, al_g["bias"])


def _run(x, h0, w_ih, w_hh, bias, gos, nonlin="none", hyper=(True, True), batch_sizes=None, unaligned=False):
    """One case through hyrnn_nets.mobius_gru_loop."""
    from hypad_amd.hyperspace import hyrnn_nets
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    d = [mk(t).requires_grad_(True) for t in (x, h0, w_ih, w_hh, bias)]
    outs, hl = hyrnn_nets.mobius_gru_loop(*d, -1.0, batch_sizes=batch_sizes, hyperbolic_input=hyper[0], hyperbolic_hidden_state0=hyper[1],
                                          nonlin=NONLINS[nonlin])
    torch.autograd.backward([outs, hl][:len(gos)], [g.cuda() for g in gos])
    return dict(outs=outs.detach().cpu(), h_last=hl.detach().cpu(), gx=d[0].grad.cpu(), gh0=d[1].grad.cpu(), gwi=d[2].grad.cpu(), gwh=d[3].grad.cpu(),
                gb=d[4].grad.cpu())


def _check(tag, got, res, T, rim=None):
    ck = Ck(tag)
    r64, r32 = res[F64], res[F32]
    if rim is not None:                                     # that row alone: its states, and its rows of grad_x and grad_h0
        for name, sel in (("outs", lambda t: t[:, rim]), ("h_last", lambda t: t[rim:rim + 1]), ("gx", lambda t: t[:, rim]), ("gh0", lambda t: t[rim:rim + 1])):
            ck.cmp(name + " (rim row)", sel(got[name]), sel(r64[name]), sel(r32[name]), steps=T)
        return ck
    for name in ("outs", "h_last", "gx", "gh0"):
        ck.cmp(name, got[name], r64[name], r32[name], steps=T)
    _reductions(ck, res, got["gwi"], got["gwh"], got["gb"])
    for name, t in got.items():
        assert bool(torch.isfinite(t).all()), (tag, name)
    return ck


# ================================================================================================ the reference's recorded cases
def test_recorded_cases_through_the_public_functions():
    from hypad_amd.hyperspace import gmath, hyrnn_nets
    from test_mobius_gru_host import BATCH_SIZES, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    prm = [fx[k] for k in ("weight_ih", "weight_hh", "bias")]
    cks = []
    for nl in NONLINS:                                       # the cell: the loop's restatement at T = 1
        d = [t.cuda().requires_grad_(True) for t in (fx["x"][0], fx["h0"], *prm)]
        out = hyrnn_nets.mobius_gru_cell(*d, torch.tensor(-1.0), nonlin=NONLINS[nl])
        assert out.shape == (9, 5)
        out.backward(fx["grad_cell"].cuda())
        got = dict(outs=out.detach().cpu()[None], h_last=out.detach().cpu(), gx=d[0].grad.cpu()[None], gh0=d[1].grad.cpu(), gwi=d[2].grad.cpu(),
                   gwh=d[3].grad.cpu(), gb=d[4].grad.cpu())
        cks.append(_check(f"recorded cell {nl}", got, _refs(None, fx["x"][:1], fx["h0"], *prm, [fx["grad_cell"][None]], nl), 1))
    got = _run(fx["x"], fx["h0"], *prm, [fx["grad_outs"]])
    assert got["outs"].shape == (4, 9, 5) and got["h_last"].shape == (9, 5)
    cks.append(_check("recorded loop, ball-valued", got, _refs(None, fx["x"], fx["h0"], *prm, [fx["grad_outs"]]), 4))
    d = [t.cuda().requires_grad_(True) for t in (fx["x_tangent"], fx["h0_tangent"], *prm)]
    outs, hl = hyrnn_nets.mobius_gru_loop(*d, -1.0)          # the defaults: Euclidean input and h0
    outs.backward(fx["grad_outs"].cuda())
    got = dict(outs=outs.detach().cpu(), h_last=hl.detach().cpu(), gx=d[0].grad.cpu(), gh0=d[1].grad.cpu(), gwi=d[2].grad.cpu(), gwh=d[3].grad.cpu(),
               gb=d[4].grad.cpu())
    cks.append(_check("recorded loop, defaults", got, _refs(None, fx["x_tangent"], fx["h0_tangent"], *prm, [fx["grad_outs"]], hyper=(False, False)), 4))
    gos = [fx["grad_packed"], fx["grad_h_last"]]
    for sizes in (BATCH_SIZES, torch.tensor(BATCH_SIZES)):
        got = _run(fx["x_packed"], fx["h0"], *prm, gos, "tanh", batch_sizes=sizes)
        assert got["outs"].shape == (27, 5) and got["h_last"].shape == (9, 5)
        cks.append(_check("recorded packed", got, _refs("packed", fx["x_packed"], fx["h0"], *prm, gos, "tanh", batch_sizes=BATCH_SIZES), 4))
    w, x = (fx[k].cuda().requires_grad_(True) for k in ("pmul_w", "pmul_x"))
    o = gmath.mobius_pointwise_mul(w, x, k=torch.tensor(-1.0))
    o.backward(fx["grad_cell"].cuda())
    assert bool((o[4] == 0).all()) and bool((w.grad[4] == 0).all()) and bool((x.grad[4] == 0).all())      # every product <= 1e-8
    cks.append(_pmul_check("recorded pointwise mul", fx["pmul_w"], fx["pmul_x"], fx["grad_cell"], o, w.grad, x.grad))
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ the sweep
@pytest.mark.parametrize("rows,I,H,T,nl", [s + ("none",) for s in SHAPES] + [s + (nl,) for s in NONLIN_SHAPES for nl in ("tanh", "relu")])
def test_gru_forward_and_backward(rows, I, H, T, nl):
    g = torch.Generator().manual_seed(1000000 * rows + 10000 * I + 100 * H + T)
    x, h0, w_ih, w_hh, bias, go = _data(g, rows, I, H, T)
    ck = _check(f"({rows},{I},{H},{T}) {nl}", _run(x, h0, w_ih, w_hh, bias, [go], nl), _refs((rows, I, H, T, nl), x, h0, w_ih, w_hh, bias, [go], nl), T)
    _report(f"({rows},{I},{H},{T}) {nl}", [ck])
    _finish([ck])


@pytest.mark.parametrize("rows,I,H,T", SHAPES)
def test_gru_rim_row(rows, I, H, T):
    """One row of x_0 and of h0 on the 1 - 1e-3 norm; its states and its rows of grad_x and grad_h0 compared alone."""
    g = torch.Generator().manual_seed(1000000 * rows + 10000 * I + 100 * H + T + 1)
    x, h0, w_ih, w_hh, bias, go = _data(g, rows, I, H, T, rim=True)
    ck = _check(f"({rows},{I},{H},{T}) rim row", _run(x, h0, w_ih, w_hh, bias, [go]), _refs(None, x, h0, w_ih, w_hh, bias, [go]), T,
                rim=1 if rows >= 3 else 0)
    _report(f"rim row ({rows},{I},{H},{T})", [ck])
    _finish([ck])


def _pmul_check(tag, w, x, go, out, gw, gx):
    res = {}
    for dt in (F64, F32):
        ww, xx = _leaf(w, dt), _leaf(x, dt)
        o = pointwise_mul_ref(ww, xx)
        gs = torch.autograd.grad(o, [ww, xx], go.to(dt))
        res[dt] = (o.detach(), gs[0], gs[1])
    ck = Ck(tag)
    ck.cmp("out", out.detach().cpu(), res[F64][0], res[F32][0])
    ck.cmp("grad_x", gx.cpu(), res[F64][2], res[F32][2])
    if w.shape == x.shape:
        ck.cmp("grad_w", gw.cpu(), res[F64][1], res[F32][1])
    else:                                                   # one row of w for every row of x: grad_w is a sum over the rows
        xx, gg = _leaf(x, F64), go.double()
        wr = w.double().expand_as(x).clone().requires_grad_(True)
        per_row = torch.autograd.grad(pointwise_mul_ref(wr, xx), wr, gg)[0]
        wr32 = w.expand_as(x).clone().requires_grad_(True)
        per_row32 = torch.autograd.grad(pointwise_mul_ref(wr32, _leaf(x, F32)), wr32, go)[0]
        ck.red("grad_w", gw.cpu().reshape(-1), per_row.sum(0), per_row.abs().sum(0), x.shape[0], sc.grad_allowance(per_row, per_row32))
    return ck


@pytest.mark.parametrize("rows,dim,w_rows", [(39, 100, 39), (17, 256, 1)])
def test_pointwise_mul_alone(rows, dim, w_rows):
    from hypad_amd.hyperspace import gmath
    g = torch.Generator().manual_seed(100 * rows + dim)
    x = _ball_rows(g, rows, dim, edge=False)
    w = torch.rand(w_rows, dim, generator=g)
    if w_rows == rows:
        w[2] = 1e-9                                         # every product <= 1e-8: the zero row
    go = torch.randn(rows, dim, generator=g)
    wd, xd = w.cuda().requires_grad_(True), x.cuda().requires_grad_(True)
    out = gmath.mobius_pointwise_mul(wd if w_rows == rows else wd[0], xd, k=-1.0)
    out.backward(go.cuda())
    if w_rows == rows:
        assert bool((out[2] == 0).all()) and bool((xd.grad[2] == 0).all())
    ck = _pmul_check(f"pointwise mul ({rows},{dim}) w_rows {w_rows}", w, x, go, out, wd.grad, xd.grad)
    _report(f"pointwise mul ({rows},{dim})", [ck])
    _finish([ck])


def test_loop_gives_the_bits_of_repeated_cell_calls():
    """Both run the same kernel body: T calls of mobius_gru_cell give, bit for bit, the outs of mobius_gru_loop over T steps; the
    gradients that flow back through the T calls agree with the restatement under the rule."""
    from hypad_amd.hyperspace import hyrnn_nets
    rows, I, H, T = 17, 33, 63, 3
    g = torch.Generator().manual_seed(1000000 * rows + 10000 * I + 100 * H + T)
    x, h0, w_ih, w_hh, bias, go = _data(g, rows, I, H, T)
    for nl in ("none", "tanh"):
        loop = _run(x, h0, w_ih, w_hh, bias, [go], nl)
        d = [t.cuda().requires_grad_(True) for t in (x, h0, w_ih, w_hh, bias)]
        h, outs = d[1], []
        for t in range(T):
            h = hyrnn_nets.mobius_gru_cell(d[0][t], h, d[2], d[3], d[4], -1.0, nonlin=NONLINS[nl])
            outs.append(h)
        outs = torch.stack(outs)
        outs.backward(go.cuda())
        assert torch.equal(outs.detach().cpu(), loop["outs"])
        plain, _ = hyrnn_nets.mobius_gru_loop(*(t.cuda() for t in (x, h0, w_ih, w_hh, bias)), -1.0, hyperbolic_input=True, hyperbolic_hidden_state0=True,
                                              nonlin=NONLINS[nl])               # no operand asks for a gradient: nothing is saved
        assert plain.grad_fn is None and torch.equal(plain.cpu(), loop["outs"])
        got = dict(outs=outs.detach().cpu(), h_last=h.detach().cpu(), gx=d[0].grad.cpu(), gh0=d[1].grad.cpu(), gwi=d[2].grad.cpu(), gwh=d[3].grad.cpu(),
                   gb=d[4].grad.cpu())
        ck = _check(f"T cell calls {nl}", got, _refs((rows, I, H, T, nl), x, h0, w_ih, w_hh, bias, [go], nl), T)
        _finish([ck])


def test_operands_at_storage_offset_1():
    rows, I, H, T = 39, 100, 100, 2
    g = torch.Generator().manual_seed(391001002)
    x, h0, w_ih, w_hh, bias, go = _data(g, rows, I, H, T)
    ck = _check("(39,100,100,2) x, h0 and the weights at storage offset 1", _run(x, h0, w_ih, w_hh, bias, [go], unaligned=True),
                _refs(None, x, h0, w_ih, w_hh, bias, [go]), T)
    _report("unaligned", [ck])
    _finish([ck])


# ================================================================================================ the C ABI directly
class _Abi:
    """One case's device buffers and the two calls."""

    def __init__(self, rows, I, H, T, nl="none", seed=0):
        self.c = _C()
        self.rows, self.I, self.H, self.T, self.nl = rows, I, H, T, CODES[nl]
        g = torch.Generator().manual_seed(1000000 * rows + 10000 * I + 100 * H + T + seed)
        self.host = _data(g, rows, I, H, T)
        self.x, self.h0, self.w_ih, self.w_hh, self.bias, self.go = (t.cuda() for t in self.host)
        self.need = self.c.lib.hypad_mobius_gru_workspace_bytes(T, rows, I, H)
        self.out = torch.empty(T, rows, H, device="cuda")
        self.saved = torch.empty(T, rows, 6 * H, device="cuda")

    def ws(self, fill=NAN):
        return torch.full((max(self.need // 4, 1),), fill, device="cuda")

    def fwd(self, out=None, saved=True, ws=None, nbytes=None, **over):
        c, a = self.c, dict(x=self.x, h0=self.h0, w_ih=self.w_ih, w_hh=self.w_hh, bias=self.bias, T=self.T, rows=self.rows, I=self.I, H=self.H, nl=self.nl)
        a.update(over)
        ws = self.ws() if ws is None else ws
        return c.lib.hypad_mobius_gru_fwd(c.ptr(a["x"]), c.ptr(a["h0"]), c.ptr(a["w_ih"]), c.ptr(a["w_hh"]), c.ptr(a["bias"]),
                                          c.ptr(self.out if out is None else out), c.ptr(self.saved) if saved else None, c.ptr(ws),
                                          self.need if nbytes is None else nbytes, a["T"], a["rows"], a["I"], a["H"], a["nl"], c.stream())

    def bwd(self, grads, ghl=None, ws=None, nbytes=None, **over):
        c, a = self.c, dict(x=self.x, h0=self.h0, w_ih=self.w_ih, w_hh=self.w_hh, bias=self.bias, go=self.go, saved=self.saved, T=self.T, rows=self.rows,
                            I=self.I, H=self.H, nl=self.nl)
        a.update(over)
        ws = self.ws() if ws is None else ws
        return c.lib.hypad_mobius_gru_bwd(c.ptr(a["x"]), c.ptr(a["h0"]), c.ptr(a["w_ih"]), c.ptr(a["w_hh"]), c.ptr(a["bias"]), c.ptr(self.out),
                                          c.ptr(a["saved"]), c.ptr(a["go"]), c.ptr(ghl), *(c.ptr(t) for t in grads), c.ptr(ws),
                                          self.need if nbytes is None else nbytes, a["T"], a["rows"], a["I"], a["H"], a["nl"], c.stream())

    def grad_shapes(self):
        return ((self.T, self.rows, self.I), (self.rows, self.H), (3 * self.H, self.I), (3 * self.H, self.H), (3, self.H))


def test_out_and_grad_x_are_written_between_their_guards():
    a = _Abi(17, 33, 63, 3)
    res = _refs((17, 33, 63, 3, "none"), *a.host[:5], [a.host[5]])
    obuf, out = _guarded((3, 17, 63), 3)
    gbuf, gx = _guarded((3, 17, 33), 5)
    a.c.check(a.fwd(out=out), "mobius_gru_fwd")
    a.out = out
    grads = [gx] + [torch.full(s, NAN, device="cuda") for s in a.grad_shapes()[1:]]
    a.c.check(a.bwd(grads), "mobius_gru_bwd")
    torch.cuda.synchronize()
    assert _guards_intact(obuf, 3) and _guards_intact(gbuf, 5)
    got = dict(outs=out.cpu(), h_last=out[-1].cpu(), gx=gx.cpu(), gh0=grads[1].cpu(), gwi=grads[2].cpu(), gwh=grads[3].cpu(), gb=grads[4].cpu())
    _finish([_check("guarded (17,33,63,3)", got, res, 3)])
    # inference (no `saved`) gives the same bits
    out2 = torch.full((3, 17, 63), NAN, device="cuda")
    a.c.check(a.fwd(out=out2, saved=False), "mobius_gru_fwd")
    assert torch.equal(out2, out)


def test_each_null_gradient_combination_and_grad_h_last():
    """Every subset of (grad_x, grad_h0, grad_w_ih, grad_w_hh, grad_bias): what is asked for has the bits of the run that asks for all.
    grad_h_last is added to the last step's gradient: the same bits as adding it to grad_out by hand."""
    a = _Abi(17, 33, 63, 3, "tanh")
    q = lambda t: torch.round(t * 1024) / 1024             # multiples of 2^-10: the sum of two of them is exact in fp32
    a.host = a.host[:5] + (q(a.host[5]),)
    a.go = a.host[5].cuda()
    a.c.check(a.fwd(), "mobius_gru_fwd")
    full = None
    for sel in range(31, -1, -1):
        outs = [torch.full(s, NAN, device="cuda") if sel >> i & 1 else None for i, s in enumerate(a.grad_shapes())]
        a.c.check(a.bwd(outs), f"mobius_gru_bwd {sel:05b}")
        if sel == 31:
            full = outs
            got = dict(outs=a.out.cpu(), h_last=a.out[-1].cpu(), gx=outs[0].cpu(), gh0=outs[1].cpu(), gwi=outs[2].cpu(), gwh=outs[3].cpu(), gb=outs[4].cpu())
            _finish([_check("C ABI (17,33,63,3) tanh", got, _refs(None, *a.host[:5], [a.host[5]], "tanh"), 3)])
        for t, f in zip(outs, full):
            assert t is None or torch.equal(t, f), f"{sel:05b}"
    ghl = q(torch.randn(17, 63, generator=torch.Generator().manual_seed(5))).cuda()
    with_hl = [torch.full(s, NAN, device="cuda") for s in a.grad_shapes()]
    a.c.check(a.bwd(with_hl, ghl=ghl), "mobius_gru_bwd")
    go2 = a.go.clone()
    go2[-1] += ghl
    by_hand = [torch.full(s, NAN, device="cuda") for s in a.grad_shapes()]
    a.c.check(a.bwd(by_hand, go=go2), "mobius_gru_bwd")
    for u, v in zip(with_hl, by_hand):
        assert bool(torch.isfinite(u).all()) and torch.equal(u, v)
    assert not torch.equal(with_hl[1], full[1])


def test_many_row_tiles_and_two_backward_runs_give_the_same_bits():
    """4 099 rows at (100, 100, 2): 257 row tiles feed every sum over rows; two runs of the backward agree bit for bit."""
    rows, I, H, T = 4099, 100, 100, 2
    g = torch.Generator().manual_seed(4099100)
    x, h0, w_ih, w_hh, bias, go = _data(g, rows, I, H, T)
    runs = []
    for _ in range(2):
        runs.append(_run(x, h0, w_ih, w_hh, bias, [go]))
        torch.full((4099 * 100 * 7,), NAN, device="cuda")   # (another history of the allocator's blocks between the runs)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    ck = _check("(4099,100,100,2)", runs[0], _refs(None, x, h0, w_ih, w_hh, bias, [go]), T)
    _report("4 099 rows", [ck])
    _finish([ck])


def test_refusals_write_nothing():
    a = _Abi(4, 8, 16, 2)
    z = lambda *s: torch.zeros(*s, device="cuda")
    out = a.out = torch.full((2, 4, 16), SENTINEL, device="cuda")
    a.saved.fill_(SENTINEL)
    grads = [torch.full(s, SENTINEL, device="cuda") for s in a.grad_shapes()]
    ws = a.ws(SENTINEL)
    fwd = lambda **kw: a.fwd(out=out, ws=ws, **kw)
    bwd = lambda **kw: a.bwd(grads, ws=ws, **kw)
    wide = dict(H=257, h0=z(4, 257), w_ih=z(771, 8), w_hh=z(771, 257), bias=z(3, 257))
    assert fwd(**wide) == HYPAD_EUNSUPPORTED and bwd(**wide) == HYPAD_EUNSUPPORTED
    wide = dict(I=257, x=z(2, 4, 257), w_ih=z(48, 257))
    assert fwd(**wide) == HYPAD_EUNSUPPORTED and bwd(**wide) == HYPAD_EUNSUPPORTED
    for call in (fwd, bwd):
        for k in ("x", "h0", "w_ih", "w_hh", "bias"):
            assert call(**{k: None}) == HYPAD_EINVAL, k
        for k, v in (("T", 0), ("rows", -1), ("I", 0), ("H", -2), ("nl", 3), ("nl", -1)):
            assert call(**{k: v}) == HYPAD_EINVAL, (k, v)
        assert call(nbytes=a.need - 4) == HYPAD_EWORKSPACE
    assert bwd(go=None) == HYPAD_EINVAL and bwd(saved=None) == HYPAD_EINVAL
    c = a.c
    pm = lambda fn, *args: fn(*(c.ptr(t) if isinstance(t, torch.Tensor) or t is None else t for t in args), c.stream())
    w, x, o = z(4, 16), z(4, 16), grads[1]
    assert pm(c.lib.hypad_mobius_pointwise_mul_fwd, w, x, o, 4, 257, 4) == HYPAD_EUNSUPPORTED
    assert pm(c.lib.hypad_mobius_pointwise_mul_fwd, None, x, o, 4, 16, 4) == HYPAD_EINVAL
    assert pm(c.lib.hypad_mobius_pointwise_mul_fwd, w, x, o, 4, 16, 2) == HYPAD_EINVAL
    assert pm(c.lib.hypad_mobius_pointwise_mul_bwd, w, x, x, None, o, 4, 16, 4) == HYPAD_EINVAL
    assert pm(c.lib.hypad_mobius_pointwise_mul_bwd, w, x, x, o, o, -1, 16, 4) == HYPAD_EINVAL
    torch.cuda.synchronize()
    for t in (out, a.saved, ws, *grads):
        assert bool((t == SENTINEL).all())                  # nothing ran
    # an empty batch: no row kernel, zero parameter gradients; the row buffers and the workspace may be NULL
    assert c.lib.hypad_mobius_gru_fwd(None, None, c.ptr(a.w_ih), c.ptr(a.w_hh), c.ptr(a.bias), None, None, None, 0, 2, 0, 8, 16, 0, c.stream()) == 0
    assert c.lib.hypad_mobius_gru_bwd(None, None, c.ptr(a.w_ih), c.ptr(a.w_hh), c.ptr(a.bias), None, None, None, None, None, None, c.ptr(grads[2]),
                                      c.ptr(grads[3]), c.ptr(grads[4]), None, 0, 2, 0, 8, 16, 0, c.stream()) == 0
    torch.cuda.synchronize()
    assert all(bool((t == 0).all()) for t in grads[2:]) and all(bool((t == SENTINEL).all()) for t in (out, grads[0], grads[1], ws))
    assert fwd() == 0 and bwd() == 0
    from hypad_amd.hyperspace import hyrnn_nets
    with pytest.raises(NotImplementedError, match="supported"):
        hyrnn_nets.mobius_gru_cell(z(4, 8), z(4, 257), z(771, 8), z(771, 257), z(3, 257), -1.0)
    # ... and through the Python functions
    d = [t.requires_grad_(True) for t in (torch.empty(3, 0, 8, device="cuda"), torch.empty(0, 16, device="cuda"), a.w_ih.clone(), a.w_hh.clone(), a.bias.clone())]
    outs, hl = hyrnn_nets.mobius_gru_loop(*d, -1.0, hyperbolic_input=True, hyperbolic_hidden_state0=True)
    assert outs.shape == (3, 0, 16) and hl.shape == (0, 16)
    outs.sum().backward()
    for t in d[2:]:
        assert t.grad is not None and bool((t.grad == 0).all())


# ================================================================================================ end to end
def test_gru_and_the_read_out_take_an_sgd_step():
    """mobius_gru_loop (T = 3, Euclidean input and h0) -> MobiusDist2Hyperplane on h_last -> cross-entropy, one SGD step of every parameter."""
    from dist2plane_ref import dist2plane_parts
    from hypad_amd.hyperspace import hyrnn_nets
    rows, I, H, T, N = 39, 33, 20, 3, 11
    g = torch.Generator().manual_seed(39332003)
    x, h0 = torch.randn(T, rows, I, generator=g) * 0.25, torch.randn(rows, H, generator=g) * 0.25
    s = 1 / H ** 0.5
    w_ih, w_hh = (torch.rand(3 * H, I, generator=g) * 2 - 1) * s, (torch.rand(3 * H, H, generator=g) * 2 - 1) * s
    bias = _ball_rows(g, 3, H, radius=0.5, edge=False, zero_row=False)
    point, tangent = _ball_rows(g, N, H, radius=0.8, edge=False, zero_row=False), torch.randn(N, H, generator=g)
    scale, target = 0.3 * torch.randn(N, generator=g), torch.randint(0, N, (rows,), generator=g)
    res = {}
    for dt in (F64, F32):
        xx, hh, p = _leaf(x, dt), _leaf(h0, dt), [_leaf(t, dt) for t in (w_ih, w_hh, bias, point, tangent, scale)]
        _, hl, _ = gru_loop_ref(xx, hh, p[0], p[1], p[2], torch.tanh, False, False)
        logits, _ = dist2plane_parts(hl, p[3], p[4], True, False, p[5])
        loss = torch.nn.functional.cross_entropy(logits, target)
        gs = torch.autograd.grad(loss, [xx, hh] + p)
        res[dt] = dict(logits=logits.detach(), loss=loss.detach(), gx=gs[0], gh0=gs[1], gp=gs[2:])
    head = hyrnn_nets.MobiusDist2Hyperplane(H, N)
    with torch.no_grad():
        head.point.copy_(point), head.tangent.copy_(tangent), head.scale.copy_(scale)
    head = head.cuda()
    gru = [torch.nn.Parameter(t.cuda()) for t in (w_ih, w_hh, bias)]
    params = gru + [head.point, head.tangent, head.scale]
    before = [q.detach().clone() for q in params]
    opt = torch.optim.SGD(params, lr=0.1)
    xd, hd = x.cuda().requires_grad_(True), h0.cuda().requires_grad_(True)
    _, hl = hyrnn_nets.mobius_gru_loop(xd, hd, *gru, -1.0, nonlin=torch.tanh)
    logits = head(hl)
    loss = torch.nn.functional.cross_entropy(logits, target.cuda())
    loss.backward()
    ck = Ck(f"mobius_gru_loop {I} -> {H} x {T} -> MobiusDist2Hyperplane {N}, rows {rows}")
    r64, r32 = res[F64], res[F32]
    ck.cmp("logits", logits.detach().cpu(), r64["logits"], r32["logits"], steps=T)
    ck.cmp("loss", loss.detach().cpu(), r64["loss"], r32["loss"], steps=T)
    ck.cmp("grad_x", xd.grad.cpu(), r64["gx"], r32["gx"], steps=T)
    ck.cmp("grad_h0", hd.grad.cpu(), r64["gh0"], r32["gh0"], steps=T)
    # the parameter gradients of a mean-reduced loss: sums of T * rows summands of size 1 / rows -- per element, the rule with the fp32
    # restatement's own error, which sums in the same precision
    for name, q, g64, g32 in zip(("w_ih", "w_hh", "bias", "point", "tangent", "scale"), params, r64["gp"], r32["gp"]):
        ck.cmp("grad_" + name, q.grad.cpu(), g64, g32, steps=T)
    opt.step()
    for q, q0 in zip(params, before):
        assert not torch.equal(q, q0) and torch.equal(q.detach(), torch.add(q0, q.grad, alpha=-0.1))
    _report("end to end", [ck])
    _finish([ck])
