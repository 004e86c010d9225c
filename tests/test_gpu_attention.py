"""Hyperbolic attention on the GPU (hypad_hyp_attention_*; gmath.hyperbolic_attention runs them) against the plain-torch restatement
of tests/attention_ref.py -- which tests/test_attention_host.py pins to the reference's own outputs -- run in fp64 and fp32 on the CPU,
under the project's rule ``Ck.cmp`` (C * err32 + F of tests/sweep_common.py, steps = 1).  No tolerance of its own.

The data.  Queries, keys and values: ``_ball_rows`` (radius <= 0.95, no rim row; the last query and the last value all zero, no zero
key), drawn one after the other from one generator, so no query coincides with a key -- the matmul form's limit near coincidence is
dist_matmul's (docs/history/geodesic_distance.md).  grad_out ~ N(0, 1), beta in {1, 8}.

Tile and chunk sizes of the kernels (csrc/attention.hip): 16 query rows a workgroup forward and for grad_q, 16 keys and values a
workgroup for their gradients, the walked operand in chunks of 64 points (16 a wave), two accumulator classes max(D, E) <= 64 / <= 128.
``EDGES`` has a shape at, below and above each: N and M 15, 16, 17 (a tile, a wave's share of a chunk) and 63, 64, 65 (a chunk); D and E
63, 65, 127, 128.  65 chunks: (1, 17, 4099, 20, 20) forward and for grad_q, (1, 4099, 17, 20, 20) for grad_keys and grad_values.
"""
import numpy as np
import pytest
import torch

from attention_ref import hyperbolic_attention_ref
from sweep_common import NAN, SENTINEL, Ck, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3                                 # include/hypad.h
BETAS = (1.0, 8.0)
SHAPES = [(1, 1, 1, 1, 1), (3, 17, 33, 20, 12), (1, 64, 100, 64, 64), (2, 65, 129, 100, 72), (1, 16, 260, 128, 128)]   # (batch, N, M, D, E)
EDGES = ([(1, n, 20, 20, 20) for n in (15, 16, 17, 63, 64, 65)] + [(1, 20, m, 20, 20) for m in (15, 16, 17, 63, 64, 65)]
         + [(1, 20, 20, d, 20) for d in (63, 65, 127, 128)]
         + [(1, 20, 20, 20, e) for e in (63, 65, 127, 128)])
NAMES = ("out", "grad_q", "grad_keys", "grad_values")
INF = float("inf")


def _C():
    from hypad_amd import _C as c
    return c


def _att():
    from hypad_amd.hyperspace import gmath
    return gmath.hyperbolic_attention


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\nhyperbolic attention {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _equal(a, b, what):
    for i, (u, v) in enumerate(zip(a, b)):
        assert (u is None and v is None) or torch.equal(u, v), f"{what}: tensor {i} differs"


def _data(batch, N, M, D, E, radius=0.95, seed=0):
    """q (batch, N, D), keys (batch, M, D), values (batch, M, E), grad_out (batch, N, E)."""
    g = torch.Generator().manual_seed(1000003 * batch + 10007 * N + 101 * M + 7 * D + E + seed)
    q = _ball_rows(g, batch * N, D, edge=False, radius=radius)
    keys = _ball_rows(g, batch * M, D, edge=False, radius=radius, zero_row=False)
    values = _ball_rows(g, batch * M, E, edge=False, radius=radius)
    return q.reshape(batch, N, D), keys.reshape(batch, M, D), values.reshape(batch, M, E), torch.randn(batch, N, E, generator=g)


def _mask_bias(g, shape, p=0.25):
    """N(0, 1) with -inf at a share p of the entries, never a whole row."""
    b = torch.randn(shape, generator=g)
    m = torch.rand(shape, generator=g) < p
    m[..., 0] = False
    return b.masked_fill(m, -INF)


_REFS = {}


def _refs(key, q, keys, values, go, beta, bias=None):
    """out and the three gradients of the restatement in fp64 and fp32 (computed once per key, never modified)."""
    if key is not None and key in _REFS:
        return _REFS[key]
    res = {}
    for dt in (F64, F32):
        leaves = [_leaf(t, dt) for t in (q, keys, values)]
        o = hyperbolic_attention_ref(*leaves, beta, bias)
        res[dt] = [o.detach()] + list(torch.autograd.grad(o, leaves, go.to(dt)))
    if key is not None:
        _REFS[key] = res
    return res


def _run(q, keys, values, go, beta, bias=None, unaligned=False):
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    d = [mk(t).requires_grad_(True) for t in (q, keys, values)]
    out = _att()(*d, -1.0, beta=beta, bias=None if bias is None else mk(bias))
    out.backward(go.cuda())
    return [out.detach()] + [t.grad for t in d]


def _check(ck, res, got):
    for name, t, r64, r32 in zip(NAMES, got, res[F64], res[F32]):
        assert bool(torch.isfinite(t).all()), (ck.case, name)
        assert t.shape == r64.shape, (ck.case, name, t.shape)
        ck.cmp(name, t.cpu(), r64, r32)


def _case(shape, beta, bias=None, tag=""):
    q, keys, values, go = _data(*shape)
    ck = Ck(f"{shape} beta {beta:g} {tag}")
    _check(ck, _refs((shape, beta, tag), q, keys, values, go, beta, bias), _run(q, keys, values, go, beta, bias))
    return ck


@pytest.mark.parametrize("shape", SHAPES + EDGES, ids=lambda s: "x".join(map(str, s)))
def test_forward_and_backward(shape):
    cks = [_case(shape, beta) for beta in BETAS]
    for ck in cks:
        _report(ck.case, [ck])
    _finish(cks)


# ================================================================================================ the reference's recorded cases
def test_recorded_cases_through_the_public_function():
    from test_attention_host import BETA, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    cks = []
    for name in ("plain", "bias"):
        bias = fx["bias"] if name == "bias" else None
        got = _run(fx["q"], fx["keys"], fx["values"], fx["grad_output"], BETA, bias)
        ck = Ck("recorded " + name)
        _check(ck, _refs(None, fx["q"], fx["keys"], fx["values"], fx["grad_output"], BETA, bias), got)
        for lab, t in zip(NAMES, got):                      # (the distance from the records themselves: printed, the rule above decides)
            rec = fx[f"{name}.{lab}"].double()
            print(f"\nrecorded {name}.{lab}: {float((t.cpu().double() - rec).abs().max()) / max(1.0, float(rec.abs().max())):.2e} from the reference's fp32 record")
        cks.append(ck)
    _report("recorded cases", cks)
    _finish(cks)


# ================================================================================================ long walks
def _sorted_keys(shape, rising):
    """Queries near the origin (radius 0.3), keys ordered by their norm: falling along M (the score, and with it the running maximum,
    rises in most chunks) or rising (the maximum is set in the first chunk)."""
    q, keys, values, go = _data(*shape)
    q = q * (0.3 / 0.95)
    order = keys[0].norm(dim=-1).argsort(descending=rising)
    return q, keys[:, order].contiguous(), values, go


@pytest.mark.parametrize("which", ["maximum rises", "maximum first", "walk over the queries"])
def test_walk_of_65_chunks_twice_the_same_bits(which):
    shape = (1, 4099, 17, 20, 20) if which == "walk over the queries" else (1, 17, 4099, 20, 20)
    data = _data(*shape) if which == "walk over the queries" else _sorted_keys(shape, which == "maximum rises")
    cks = []
    for beta in BETAS:
        got = []
        for _ in range(2):
            got.append(_run(*data, beta))
            torch.full((4099 * 20 * 7,), NAN, device="cuda")    # (another history of the allocator's blocks between the runs)
        _equal(got[0], got[1], f"{shape} {which}")
        ck = Ck(f"{shape} beta {beta:g}: {which}")
        _check(ck, _refs(None, *data, beta), got[0])
        _report(ck.case, [ck])
        cks.append(ck)
    _finish(cks)


# ================================================================================================ other numeric cases
def test_scores_that_underflow_stay_finite():
    """beta = 20 and a query on the 1 - 1e-3 norm: its distances reach 7 and more, exp(s - max) leaves fp32 for most keys."""
    shape, beta = (2, 17, 33, 20, 12), 20.0
    q, keys, values, go = _data(*shape)
    v = q[0, 1].double()
    q[0, 1] = (v * ((1 - 1e-3) / float(v.norm()))).float()
    got = _run(q, keys, values, go, beta)
    ck = Ck(f"{shape} beta 20, a rim query")
    _check(ck, _refs(None, q, keys, values, go, beta), got)
    _report(ck.case, [ck])
    _finish([ck])


def test_shared_and_batched_bias_with_masked_entries():
    shape = (3, 17, 33, 20, 12)
    g = torch.Generator().manual_seed(5)
    cks = []
    for tag, bshape in (("bias (N, M)", shape[1:3]), ("bias (batch, N, M)", shape[:3])):
        bias = _mask_bias(g, bshape)
        assert bool(torch.isneginf(bias).any())
        for beta in BETAS:
            cks.append(_case(shape, beta, bias, tag))
    _report("bias with -inf", cks)
    _finish(cks)


def test_causal_mask_across_a_tile_edge():
    shape = (2, 65, 65, 20, 20)
    bias = torch.zeros(65, 65).masked_fill(torch.ones(65, 65, dtype=torch.bool).triu(1), -INF)
    cks = [_case(shape, beta, bias, "causal") for beta in BETAS]
    q, keys, values, go = _data(*shape)
    out = _run(q, keys, values, go, 1.0, bias)[0]
    first = hyperbolic_attention_ref(q[:, :1].double(), keys[:, :1].double(), values[:, :1].double())     # query 0 sees value 0 alone
    ck = Ck("causal, query 0")
    ck.cmp("out", out[:, :1].cpu(), first, hyperbolic_attention_ref(q[:, :1], keys[:, :1], values[:, :1]))
    _report("causal mask", cks + [ck])
    _finish(cks + [ck])


def test_a_fully_masked_row_is_the_origin_and_adds_nothing():
    """The last query's every score is -inf: its output and its grad_q are exactly zero, and every other number has the bits of the run
    without that query (the row is the last one, so the other rows keep their places in the tiles and the sums their order)."""
    shape, beta = (2, 9, 11, 20, 12), 1.7
    q, keys, values, go = _data(*shape)
    g = torch.Generator().manual_seed(17)
    bias = _mask_bias(g, (9, 11))
    bias[-1] = -INF
    out, gq, gk, gv = _run(q, keys, values, go, beta, bias)
    for t in (out, gq, gk, gv):
        assert bool(torch.isfinite(t).all())
    assert bool((out[:, -1] == 0).all()) and bool((gq[:, -1] == 0).all())
    out2, gq2, gk2, gv2 = _run(q[:, :-1].contiguous(), keys, values, go[:, :-1].contiguous(), beta, bias[:-1].contiguous())
    _equal([out[:, :-1], gq[:, :-1], gk, gv], [out2, gq2, gk2, gv2], "the run without the masked query")
    ck = Ck(f"{shape} with a masked query")
    _check(ck, _refs(None, q, keys, values, go, beta, bias), [out, gq, gk, gv])
    _report(ck.case, [ck])
    _finish([ck])


def test_batch_dimensions_and_operands_without_them():
    """Leading batch dimensions (2, 3) on all operands; then each operand in turn without them: it is expanded on the host and autograd
    sums its gradient over the batch.  The bias is (N, M) in one run and (2, 3, N, M) in another."""
    g = torch.Generator().manual_seed(29)
    N, M, D, E = 4, 7, 5, 6
    q = _ball_rows(g, 6 * N, D, edge=False).reshape(2, 3, N, D)
    keys = _ball_rows(g, 6 * M, D, edge=False, zero_row=False).reshape(2, 3, M, D)
    values = _ball_rows(g, 6 * M, E, edge=False).reshape(2, 3, M, E)
    go = torch.randn(2, 3, N, E, generator=g)
    b2, b4 = _mask_bias(g, (N, M)), _mask_bias(g, (2, 3, N, M))
    cks = []
    for tag, ops, bias in (("all", (q, keys, values), None), ("q shared", (q[0, 0], keys, values), b2), ("keys shared", (q, keys[0, 0], values), b4),
                           ("values shared", (q, keys, values[0, 0]), None), ("keys and values shared", (q, keys[1, 2], values[1, 2]), b2)):
        got = _run(*ops, go, 1.7, bias)
        assert got[0].shape == (2, 3, N, E) and all(t.shape == o.shape for t, o in zip(got[1:], ops))
        ck = Ck("batch dims, " + tag)
        _check(ck, _refs(None, *ops, go, 1.7, bias), got)
        cks.append(ck)
    _report("batch dims", cks)
    _finish(cks)


def test_gru_states_through_attention_to_the_read_out():
    """mobius_gru_loop (T = 2: its two steps are the two batch elements) gives the queries, keys and values -> hyperbolic_attention ->
    MobiusDist2Hyperplane -> cross-entropy at (batch, N, M, D, E) = (2, 9, 11, 20, 20): every parameter's gradient."""
    from dist2plane_ref import dist2plane_parts
    from hypad_amd.hyperspace import hyrnn_nets
    from mobius_gru_ref import gru_loop_ref
    batch, N, M, H, I, C, beta = 2, 9, 11, 20, 13, 5, 1.7
    rows = N + 2 * M
    g = torch.Generator().manual_seed(290511)
    x, h0 = torch.randn(batch, rows, I, generator=g) * 0.5, torch.randn(rows, H, generator=g) * 0.5
    s = 1 / H ** 0.5
    w_ih, w_hh = (torch.rand(3 * H, I, generator=g) * 2 - 1) * s, (torch.rand(3 * H, H, generator=g) * 2 - 1) * s
    gbias = _ball_rows(g, 3, H, radius=0.5, edge=False, zero_row=False)
    point, tangent = _ball_rows(g, C, H, radius=0.8, edge=False, zero_row=False), torch.randn(C, H, generator=g)
    scale, target = 0.3 * torch.randn(C, generator=g), torch.randint(0, C, (batch * N,), generator=g)
    names = ("x", "h0", "w_ih", "w_hh", "bias", "point", "tangent", "scale")
    res = {}
    for dt in (F64, F32):
        p = {n: _leaf(t, dt) for n, t in zip(names, (x, h0, w_ih, w_hh, gbias, point, tangent, scale))}
        outs, _, _ = gru_loop_ref(p["x"], p["h0"], p["w_ih"], p["w_hh"], p["bias"], torch.tanh, False, False)
        mid = hyperbolic_attention_ref(outs[:, :N], outs[:, N:N + M], outs[:, N + M:], beta)
        logits, _ = dist2plane_parts(mid.reshape(batch * N, H), p["point"], p["tangent"], True, False, p["scale"])
        loss = torch.nn.functional.cross_entropy(logits, target)
        gs = torch.autograd.grad(loss, [p[n] for n in names])
        res[dt] = dict(mid=mid.detach(), logits=logits.detach(), loss=loss.detach(), **{"g_" + n: v for n, v in zip(names, gs)})
    head = hyrnn_nets.MobiusDist2Hyperplane(H, C)
    with torch.no_grad():
        head.point.copy_(point), head.tangent.copy_(tangent), head.scale.copy_(scale)
    head = head.cuda()
    d = {n: t.cuda().requires_grad_(True) for n, t in zip(names[:5], (x, h0, w_ih, w_hh, gbias))}
    outs, _ = hyrnn_nets.mobius_gru_loop(d["x"], d["h0"], d["w_ih"], d["w_hh"], d["bias"], -1.0, nonlin=torch.tanh)
    mid = _att()(outs[:, :N], outs[:, N:N + M], outs[:, N + M:], -1.0, beta=beta)
    logits = head(mid.reshape(batch * N, H))
    loss = torch.nn.functional.cross_entropy(logits, target.cuda())
    loss.backward()
    ck = Ck("gru -> attention -> read-out (2, 9, 11, 20, 20)")
    r64, r32 = res[F64], res[F32]
    got = [("mid", mid.detach()), ("logits", logits.detach()), ("loss", loss.detach())] + [("g_" + n, d[n].grad) for n in names[:5]]
    got += [("g_point", head.point.grad), ("g_tangent", head.tangent.grad), ("g_scale", head.scale.grad)]
    for name, t in got:
        assert bool(torch.isfinite(t).all()), name
        ck.cmp(name, t.cpu(), r64[name], r32[name])
    _report(ck.case, [ck])
    _finish([ck])


# ================================================================================================ the same bits
def test_operands_at_storage_offset_1_give_the_same_bits():
    shape = (2, 65, 129, 100, 72)
    q, keys, values, go = _data(*shape)
    bias = _mask_bias(torch.Generator().manual_seed(3), shape[1:3])
    _equal(_run(q, keys, values, go, 1.0, bias), _run(q, keys, values, go, 1.0, bias, unaligned=True), "storage offset 1")


def _abi_fwd(c, q, keys, values, bias, beta, out, saved, lse):
    batch, N, D = q.shape
    M, E = values.shape[1:]
    stride = 0 if bias is None or bias.dim() == 2 else N * M
    return c.lib.hypad_hyp_attention_fwd(c.ptr(q), c.ptr(keys), c.ptr(values), c.ptr(bias), stride, beta, c.ptr(out), c.ptr(saved), c.ptr(lse), batch,
                                         N, M, D, E, c.stream())


def _abi_bwd(c, q, keys, values, bias, beta, saved, lse, go, gq, gk, gv):
    batch, N, D = q.shape
    M, E = values.shape[1:]
    stride = 0 if bias is None or bias.dim() == 2 else N * M
    nbytes = c.lib.hypad_hyp_attention_workspace_bytes(batch, N, M, D, E)
    assert nbytes == 4 * batch * N * (E + 2)
    ws = torch.empty(max(nbytes // 4, 1), device="cuda")
    return c.lib.hypad_hyp_attention_bwd(c.ptr(q), c.ptr(keys), c.ptr(values), c.ptr(bias), stride, beta, c.ptr(saved), c.ptr(lse), c.ptr(go),
                                         c.ptr(gq), c.ptr(gk), c.ptr(gv), c.ptr(ws), nbytes, batch, N, M, D, E, c.stream())


def test_each_null_gradient_combination_and_inference_have_the_bits_of_the_full_run():
    c = _C()
    shape, beta = (2, 65, 70, 20, 12), 1.7
    batch, N, M, D, E = shape
    q, keys, values, go = (t.cuda() for t in _data(*shape))
    bias = _mask_bias(torch.Generator().manual_seed(4), (batch, N, M)).cuda()
    out, saved, lse = torch.full((batch, N, E), NAN, device="cuda"), torch.full((batch, N, E + 1), NAN, device="cuda"), torch.full((batch, N), NAN, device="cuda")
    c.check(_abi_fwd(c, q, keys, values, bias, beta, out, saved, lse), "fwd")
    inference = torch.full((batch, N, E), NAN, device="cuda")
    c.check(_abi_fwd(c, q, keys, values, bias, beta, inference, None, None), "fwd, inference")
    assert torch.equal(out, inference) and bool(torch.isfinite(saved).all()) and bool(torch.isfinite(lse).all())
    full = None
    for sel in (7, 6, 5, 4, 3, 2, 1, 0):
        outs = [torch.full(tuple(t.shape), NAN, device="cuda") if sel >> i & 1 else None for i, t in enumerate((q, keys, values))]
        c.check(_abi_bwd(c, q, keys, values, bias, beta, saved, lse, go, *outs), f"bwd {sel:03b}")
        full = full or outs
        _equal([t for t in outs if t is not None], [f for t, f in zip(outs, full) if t is not None], f"bwd {sel:03b}")
    assert all(bool(torch.isfinite(t).all()) for t in full)
    # through the Python function: no operand asks for a gradient -> nothing is saved, the same output
    plain = _att()(q, keys, values, -1.0, beta=beta, bias=bias)
    assert plain.grad_fn is None and torch.equal(plain, out)
    qd = q.clone().requires_grad_(True)
    only_q = _att()(qd, keys, values, -1.0, beta=torch.tensor(beta, dtype=F64), bias=bias)      # (an fp32 tensor would hold another beta)
    only_q.backward(go)
    assert torch.equal(only_q.detach(), out) and torch.equal(qd.grad, full[0])


# ================================================================================================ the C ABI directly
def test_results_are_written_between_their_guards():
    c = _C()
    cks = []
    for shape, beta in (((2, 17, 33, 20, 12), 1.0), ((1, 65, 63, 127, 65), 8.0)):
        batch, N, M, D, E = shape
        q, keys, values, go = _data(*shape)
        bias = _mask_bias(torch.Generator().manual_seed(6), (N, M))
        res = _refs(None, q, keys, values, go, beta, bias)
        dev = [t.cuda() for t in (q, keys, values, bias, go)]
        offs = (3, 1, 2, 5, 7, 1)
        bufs = [_guarded(s, o) for s, o in zip(((batch, N, E), (batch, N, E + 1), (batch, N), (batch, N, D), (batch, M, D), (batch, M, E)), offs)]
        (_, out), (_, saved), (_, lse), (_, gq), (_, gk), (_, gv) = bufs
        c.check(_abi_fwd(c, *dev[:4], beta, out, saved, lse))
        c.check(_abi_bwd(c, *dev[:4], beta, saved, lse, dev[4], gq, gk, gv))
        torch.cuda.synchronize()
        for (buf, v), off in zip(bufs, offs):
            assert _guards_intact(buf, off) and bool(torch.isfinite(v).all())
        ck = Ck(f"guarded {shape}")
        _check(ck, res, [out, gq, gk, gv])
        cks.append(ck)
    _report("guarded", cks)
    _finish(cks)


def test_refusals_write_nothing():
    c = _C()
    L = c.lib
    batch, N, M = 2, 4, 6
    for D, E in ((129, 8), (8, 129), (8, 8)):
        z = lambda *s: torch.zeros(s, device="cuda")
        q, keys, values, go, saved, lse = z(batch, N, D), z(batch, M, D), z(batch, M, E), z(batch, N, E), z(batch, N, E + 1), z(batch, N)
        out, gq, gk, gv = (torch.full(s, SENTINEL, device="cuda") for s in ((batch, N, E), (batch, N, D), (batch, M, D), (batch, M, E)))
        ws = torch.empty(batch * N * (E + 2), device="cuda")

        def fwd(a=q, k=keys, v=values, o=out, b=batch, n=N, m=M, d=D, e=E, beta=1.0, sv=None, ls=None):
            return L.hypad_hyp_attention_fwd(c.ptr(a), c.ptr(k), c.ptr(v), None, 0, beta, c.ptr(o), c.ptr(sv), c.ptr(ls), b, n, m, d, e, c.stream())

        def bwd(a=q, k=keys, v=values, sv=saved, ls=lse, g=go, b=batch, n=N, m=M, d=D, e=E, beta=1.0, w=ws, wb=4 * batch * N * (E + 2)):
            return L.hypad_hyp_attention_bwd(c.ptr(a), c.ptr(k), c.ptr(v), None, 0, beta, c.ptr(sv), c.ptr(ls), c.ptr(g), c.ptr(gq), c.ptr(gk),
                                             c.ptr(gv), c.ptr(w), wb, b, n, m, d, e, c.stream())

        if (D, E) != (8, 8):
            assert fwd() == bwd() == HYPAD_EUNSUPPORTED
        else:
            assert fwd(a=None) == fwd(k=None) == fwd(v=None) == fwd(o=None) == fwd(sv=saved) == fwd(ls=lse) == HYPAD_EINVAL
            assert bwd(a=None) == bwd(k=None) == bwd(v=None) == bwd(sv=None) == bwd(ls=None) == bwd(g=None) == HYPAD_EINVAL
            for call in (fwd, bwd):
                assert call(b=-1) == call(n=-1) == call(m=-2) == call(m=0) == call(d=0) == call(e=-3) == HYPAD_EINVAL
                assert call(beta=INF) == call(beta=NAN) == HYPAD_EINVAL
                assert call(b=2 ** 20, n=2 ** 6, m=2 ** 5) == HYPAD_EUNSUPPORTED      # 2^31 pairs
            assert bwd(w=None) == bwd(wb=4 * batch * N * (E + 2) - 4) == -2               # HYPAD_EWORKSPACE
        torch.cuda.synchronize()
        for t in (out, gq, gk, gv):
            assert bool((t == SENTINEL).all())              # nothing ran
    assert fwd(sv=saved, ls=lse) == 0 and bwd() == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any()) and not bool((gk == SENTINEL).any())
    with pytest.raises(NotImplementedError, match="supported"):
        _att()(torch.zeros(2, 4, 129, device="cuda"), torch.zeros(2, 3, 129, device="cuda"), torch.zeros(2, 3, 8, device="cuda"), -1.0)


def test_no_queries_leave_zero_gradients():
    c = _C()
    L = c.lib
    keys, values = torch.zeros(2, 6, 8, device="cuda"), torch.zeros(2, 6, 5, device="cuda")
    gk, gv = torch.full((2, 6, 8), NAN, device="cuda"), torch.full((2, 6, 5), NAN, device="cuda")
    assert L.hypad_hyp_attention_fwd(None, c.ptr(keys), c.ptr(values), None, 0, 1.0, None, None, None, 2, 0, 6, 8, 5, c.stream()) == 0
    assert L.hypad_hyp_attention_bwd(None, c.ptr(keys), c.ptr(values), None, 0, 1.0, None, None, None, None, c.ptr(gk), c.ptr(gv), None, 0, 2, 0, 6, 8, 5,
                                     c.stream()) == 0
    assert bool((gk == 0).all()) and bool((gv == 0).all())
    assert L.hypad_hyp_attention_fwd(None, None, None, None, 0, 1.0, None, None, None, 0, 4, 6, 8, 5, c.stream()) == 0
    q, kd, vd = torch.zeros(2, 0, 8, device="cuda").requires_grad_(True), keys.requires_grad_(True), values.requires_grad_(True)
    out = _att()(q, kd, vd, -1.0)
    assert out.shape == (2, 0, 5)
    out.sum().backward()
    assert bool((kd.grad == 0).all()) and bool((vd.grad == 0).all()) and q.grad.shape == (2, 0, 8)


# ================================================================================================ side stream, captured graph
def _fwd_bwd(q, keys, values, go, bias, beta):
    out = _att()(q, keys, values, -1.0, beta=beta, bias=bias)
    return (out,) + torch.autograd.grad(out, [q, keys, values], go)


def _stream_case():
    shape = (2, 65, 129, 100, 72)
    return _data(*shape) + (_mask_bias(torch.Generator().manual_seed(8), shape[1:3]),)


def _on_device(host):
    q, keys, values, go, bias = (t.cuda() for t in host)
    return q.requires_grad_(True), keys.requires_grad_(True), values.requires_grad_(True), go, bias


def test_on_a_side_stream():
    host = _stream_case()
    want = [t.clone() for t in _fwd_bwd(*_on_device(host), 1.7)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _fwd_bwd(*_on_device(host), 1.7)              # placed and filled on the side stream: a launch on stream 0 would race them
    side.synchronize()
    _equal(got, want, "on a side stream")


def test_captured_and_replayed_with_changed_inputs():
    host = _stream_case()
    g = torch.Generator().manual_seed(11)
    second = (host[0].flip(0).contiguous(), (host[1] * 0.5).contiguous(), (host[2] * 0.75).contiguous(), torch.randn(host[3].shape, generator=g),
              _mask_bias(g, host[4].shape))
    wants = [[t.clone() for t in _fwd_bwd(*_on_device(h), 1.7)] for h in (host, second)]
    assert not torch.equal(wants[0][0], wants[1][0])
    static = _on_device(host)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _fwd_bwd(*static, 1.7)                              # the eager warm-up, on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        outs = _fwd_bwd(*static, 1.7)
    for i in (1, 0):                                        # replayed twice, each time with other inputs
        with torch.no_grad():
            for s, h in zip(static, (host, second)[i]):
                s.copy_(h.cuda())
        graph.replay()
        torch.cuda.synchronize()
        _equal([t.detach() for t in outs], wants[i], f"replay with data set {i}")


# ================================================================================================ memory
def test_no_n_by_m_tensor_is_allocated():
    """(2, 1024, 1024, 32, 32): one (batch, N, M) fp32 tensor is 8 MiB.  The operands, output, gradients, saved rows and workspace of the
    fused function are about 3 MiB; its forward plus backward must stay below the 8 MiB, and the composition must not."""
    from hypad_amd.hyperspace import gmath
    shape, beta = (2, 1024, 1024, 32, 32), 1.7
    host = _data(*shape)
    limit = 4 * shape[0] * shape[1] * shape[2]

    def rise(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        q, keys, values, go = (t.cuda() for t in host)
        q.requires_grad_(True), keys.requires_grad_(True), values.requires_grad_(True)
        out = fn(q, keys, values)
        out.backward(go)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        assert bool(torch.isfinite(out).all()) and all(bool(torch.isfinite(t.grad).all()) for t in (q, keys, values))
        return peak, out.detach().cpu()

    fused, out_f = rise(lambda q, k, v: gmath.hyperbolic_attention(q, k, v, -1.0, beta=beta))
    composed, out_c = rise(lambda q, k, v: gmath.weighted_midpoint_bmm(v, torch.softmax(-beta * gmath.dist_matmul(q, k.transpose(-1, -2), -1.0), -1), -1.0))
    print(f"\nforward + backward at {shape}: fused {fused / 2 ** 20:.2f} MiB, composed {composed / 2 ** 20:.2f} MiB, one (batch, N, M) tensor "
          f"{limit / 2 ** 20:.0f} MiB; fused against composed output {float((out_f - out_c).abs().max()):.2e}")
    assert fused < limit < composed
