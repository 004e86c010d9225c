"""The dense building blocks of the differentiable path (csrc/ops_dense.hip; hypad_amd/autograd.py and hyperspace/hyrnn_nets.py run
them, bench.py's roofline_lstm section times them) against plain fp64 torch on the CPU, at the shapes where their launch code
takes another path: the weights-stationary LSTM layer past one tile per wave, every k-group count and wave count of its generic
form, misaligned buffers, both sides of the switch from the streamed form; the Moebius head backward and the column sum at every row
layout; mobius_linear and linear + activation at the edges of gemm_nt (weight-load width 4 / 2 / 1, 32-k slabs, 128-k super-chunks,
output widths that are no multiple of 16) and of outer_sum_kernel (four-row steps, partial tiles); the argument checks and the
empty batch.

Two rules.

Per-row quantities (forward outputs, saved gates, input gradients, the per-row bias gradients of the head) go under
``sweep_common.Checker.cmp``: errgpu <= C * err32 + F with that file's C and F, err32 being the error of the same operation run in
fp32 on the CPU.

A sum over rows (grad_w and grad_b of outer_sum_kernel, grad_bias through hypad_column_sum, the LSTM's parameter gradients) has no
such yardstick -- a second fp32 sum in another order says nothing about this one -- so it gets the running-error bound of a sum of
``rows`` products taken in ANY order: element-wise

    |got - ref64| <= summand_allowance + (rows + 4) * 2^-24 * sum_r |a_r * b_r|

(rows - 1 additions, one rounding per product, three to spare for the fused forms of the matrix pipe), the sum of absolute terms in
fp64 from the reference operands, both sides divided by max(1, max|ref64|) as in the Checker.  ``summand_allowance`` is what the
Checker rule allows the summed operand itself (``sweep_common.grad_allowance`` of a = grad_pre / grad_u / grad_gates, from its fp64
and fp32 references) times the largest |b| it is multiplied with; it is zero where the summands are the call's own inputs.  At 39
rows a dropped or doubled row is three orders of magnitude beyond this.
"""
import pytest
import torch

import sweep_common as sc
from sweep_common import NAN, SENTINEL, Ck, _at_offset, _ball_rows, _guarded, _guards_intact, _leaf, _unaligned
from oracle import gmath as og

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_EINVAL, HYPAD_EWORKSPACE, HYPAD_EUNSUPPORTED = -1, -2, -3          # include/hypad.h


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _nan(*shape):
    return torch.full(shape, NAN, device="cuda")


# ================================================================================================ A. weights-stationary LSTM layer
R = 66133                     # 4 134 tiles, the last one of 5 rows: every wave of the 128 x NW grid takes two to five tiles
REFERENCE_LAYERS = [(128, 64), (50, 64), (100, 50)]
# generic form: (K, H) -> k-groups of 16 / unit blocks
GENERIC_LAYERS = [(5, 33),    # KG 1; three unit blocks, the last unpaired
                  (33, 7),    # KG 3; one block
                  (65, 48),   # KG 5
                  (96, 16),   # KG 6: the last width on 16 waves; non-temporal gate stores
                  (97, 64),   # KG 7: the first width on 8 waves; K odd: scalar x loads
                  (100, 64),  # KG 7
                  (128, 50)]  # KG 8


def _waves(K, H, saved):
    """Waves per workgroup of the weights-stationary launch (hypad_lstm_bidir_fwd)."""
    if (K, H) in ((100, 50), (128, 64), (50, 64)):
        return 8 if (K, H) == (50, 64) and saved else 16
    return 8 if (K + 15) // 16 >= 7 else 16


def _lstm_graph(x, p, H):
    """One bidirectional layer at T = 1 from a zero state, written out: x W^T + b_ih + b_hh -> sigma(i), tanh(g), sigma(o) ->
    h = sigma(o) tanh(sigma(i) tanh(g)).  Returns out (rows, 2H), the gates in the stored order [i | g | o | tanh c] per direction
    (rows, 8H), and the two pre-activations (rows, 4H) in PyTorch's gate order."""
    outs, gates, pres = [], [], []
    for d in range(2):
        w, bi, bh = p[3 * d:3 * d + 3]
        pre = x @ w.t() + bi + bh
        i, g, o = torch.sigmoid(pre[:, :H]), torch.tanh(pre[:, 2 * H:3 * H]), torch.sigmoid(pre[:, 3 * H:])
        tc = torch.tanh(i * g)
        outs.append(o * tc)
        gates.append(torch.cat([i, g, o, tc], 1))
        pres.append(pre)
    return torch.cat(outs, 1), torch.cat(gates, 1), pres


_LSTM_REF = {}                # one entry: the tests below take their (K, H, rows) in runs


def _lstm_ref(K, H, rows):
    """Data, parameters (nn.LSTM's initialisation range) and the fp64 / fp32 results of layer (K, H) at ``rows`` rows."""
    key = (K, H, rows)
    if key not in _LSTM_REF:
        _LSTM_REF.clear()
        g = torch.Generator().manual_seed(1000 * K + H + rows)
        x = torch.randn(rows, K, generator=g)
        bound = 1.0 / H ** 0.5
        shapes = [(4 * H, K), (4 * H,), (4 * H,)] * 2
        params = [(torch.rand(*s, generator=g) * 2 - 1) * bound for s in shapes]
        go = torch.randn(rows, 2 * H, generator=g)
        ref = dict(x=x, params=params, go=go)
        for dt in (F64, F32):
            xx = _leaf(x, dt)
            pp = [_leaf(t, dt) for t in params]
            out, gates, pres = _lstm_graph(xx, pp, H)
            gr = torch.autograd.grad(out, [xx] + pres + [pp[0], pp[1], pp[3], pp[4]], go.to(dt))
            ref[dt] = dict(out=out.detach(), gates=gates.detach(), gx=gr[0], gg=torch.cat([gr[1], gr[2]], 1), gw=(gr[3], gr[5]), gb=(gr[4], gr[6]))
        _LSTM_REF[key] = ref
    return _LSTM_REF[key]


def _lstm_fwd(x, dp, out, gates, rows, K, H):
    c = _C()
    c.check(c.lib.hypad_lstm_bidir_fwd(c.ptr(x), *[c.ptr(t) for t in dp], c.ptr(out), c.ptr(gates), rows, K, H, c.stream()), "lstm_bidir_fwd")


def _lstm_param_grads(ck, ref, gg_gpu, rows, K, H, gw_gpu=None, gb_gpu=None):
    """The parameter gradients under the reduction rule: formed on the host in fp64 from the GPU's grad_gates (gw_gpu = None), or the
    GPU's own sums."""
    r64, r32 = ref[F64], ref[F32]
    x64 = ref["x"].double()
    allow_gg = sc.grad_allowance(r64["gg"], r32["gg"])
    xmax = float(x64.abs().max())
    gg3 = None if gg_gpu is None else gg_gpu.cpu().double().view(rows, 2, 4 * H)
    a64 = r64["gg"].view(rows, 2, 4 * H)
    for d, tag in enumerate(("forward", "reverse")):
        gw = gg3[:, d].t() @ x64 if gw_gpu is None else gw_gpu[d]
        gb = gg3[:, d].sum(0) if gb_gpu is None else gb_gpu[d]
        ck.red(f"grad weight_ih {tag}", gw, r64["gw"][d], a64[:, d].abs().t() @ x64.abs(), rows, allow_gg * xmax)
        ck.red(f"grad bias {tag}", gb, r64["gb"][d], a64[:, d].abs().sum(0), rows, allow_gg)


# (the three reference layers aligned and misaligned; (100, 50) last: the autograd test below shares its reference)
LSTM_R_CASES = [(K, H, False) for K, H in GENERIC_LAYERS] + [(K, H, m) for K, H in REFERENCE_LAYERS for m in (False, True)]


@pytest.mark.parametrize("K,H,misaligned", LSTM_R_CASES, ids=lambda v: str(v))
def test_weights_stationary_lstm_layer_past_one_tile_per_wave(K, H, misaligned):
    """66 133 rows: the persistent tile loop takes its second to fifth iteration (software prefetch, in-place replacement of the x
    registers, the repeated last tile, the slab reuse and the per-tile descriptors of a ragged tile that is not a wave's first).
    misaligned: x, out and gates_save at storage offset 1 (4-byte aligned: scalar x loads, no non-temporal and no 16-byte gate
    stores), with a guard float on both sides of each output."""
    c = _C()
    ref = _lstm_ref(K, H, R)
    r64, r32 = ref[F64], ref[F32]
    dp = [t.cuda() for t in ref["params"]]
    off = 1 if misaligned else 16
    x = _unaligned(ref["x"].cuda()) if misaligned else ref["x"].cuda()
    obuf, out = _guarded((R, 2 * H), off)
    gbuf, gates = _guarded((R, 8 * H), off)
    o2buf, out2 = _guarded((R, 2 * H), off)
    _lstm_fwd(x, dp, out, gates, R, K, H)
    _lstm_fwd(x, dp, out2, None, R, K, H)
    torch.cuda.synchronize()
    assert _guards_intact(obuf, off) and _guards_intact(gbuf, off) and _guards_intact(o2buf, off)
    ck = Ck(f"lstm ({K},{H}) rows {R}{' misaligned' if misaligned else ''}", tiles=(R, _waves(K, H, True)))
    ck2 = Ck(f"lstm ({K},{H}) rows {R}{' misaligned' if misaligned else ''} without saved gates", tiles=(R, _waves(K, H, False)))
    assert bool(torch.isfinite(gates).all()), "a (row, direction, gate, unit) of gates_save was not written"
    ck.cmp("out", out.cpu(), r64["out"], r32["out"])
    ck.cmp("gates_save [i | g | o | tanh c] x 2", gates.cpu(), r64["gates"], r32["gates"])
    ck2.cmp("out", out2.cpu(), r64["out"], r32["out"])
    same = torch.equal(out, out2)
    if not misaligned:
        gg, gx = _nan(R, 8 * H), _nan(R, K)
        c.check(c.lib.hypad_lstm_bidir_bwd(c.ptr(dp[0]), c.ptr(dp[3]), c.ptr(gates), c.ptr(ref["go"].cuda()), c.ptr(gg), c.ptr(gx), R, K, H,
                                           c.stream()), "lstm_bidir_bwd")
        ck.cmp("grad_x", gx.cpu(), r64["gx"], r32["gx"])
        ck.cmp("grad_gates", gg.cpu(), r64["gg"], r32["gg"])
        ggv = gg.view(R, 2, 4, H)
        assert bool((ggv[:, :, 1] == 0).all()), "the f-gate block of grad_gates is not identically zero"
        _lstm_param_grads(ck, ref, gg, R, K, H)
    ck.report()
    _finish([ck, ck2])
    assert same, "out differs between the runs with and without saved gates"


def test_lstm_layer_autograd_function_past_one_tile_per_wave():
    """autograd.lstm_layer on torch.nn.LSTM(100, 50, bidirectional=True) at 66 133 rows: out, x.grad and the gradients of weight_ih,
    bias_ih and bias_hh of both directions (outer_sum_kernel over 66 133 rows); weight_hh gradients are exactly zero."""
    from hypad_amd import autograd as hag
    K, H = 100, 50
    ref = _lstm_ref(K, H, R)
    r64, r32 = ref[F64], ref[F32]
    lstm = torch.nn.LSTM(K, H, bidirectional=True)
    names = ["weight_ih_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse"]
    with torch.no_grad():
        for n, t in zip(names, ref["params"]):
            getattr(lstm, n).copy_(t)
    lstm = lstm.cuda()
    x = ref["x"].cuda().requires_grad_(True)
    out = hag.lstm_layer(x, lstm, 0)
    out.backward(ref["go"].cuda())
    ck = Ck(f"autograd.lstm_layer ({K},{H}) rows {R}", tiles=(R, _waves(K, H, True)))
    ck.cmp("out", out.detach().cpu(), r64["out"], r32["out"])
    ck.cmp("x.grad", x.grad.cpu(), r64["gx"], r32["gx"])
    g = lambda n: getattr(lstm, n).grad.cpu()
    _lstm_param_grads(ck, ref, None, R, K, H, gw_gpu=(g("weight_ih_l0"), g("weight_ih_l0_reverse")), gb_gpu=(g("bias_ih_l0"), g("bias_ih_l0_reverse")))
    assert torch.equal(g("bias_hh_l0"), g("bias_ih_l0")) and torch.equal(g("bias_hh_l0_reverse"), g("bias_ih_l0_reverse"))
    assert bool((g("weight_hh_l0") == 0).all()) and bool((g("weight_hh_l0_reverse") == 0).all())
    ck.report()
    _finish([ck])


@pytest.mark.parametrize("K,H", [(100, 50), (20, 64)])
def test_lstm_layer_both_sides_of_the_form_switch(K, H):
    """2 047 rows run the streamed lstm_fwd_kernel, 2 048 rows the weights-stationary form: rows 0 .. 2 046 of both obey the rule
    against the same fp64 reference."""
    ref = _lstm_ref(K, H, 2048)
    r64, r32 = ref[F64], ref[F32]
    dp = [t.cuda() for t in ref["params"]]
    x = ref["x"].cuda()
    cks = []
    for rows in (2047, 2048):
        out, gates = _nan(rows, 2 * H), _nan(rows, 8 * H)
        _lstm_fwd(x[:rows].contiguous(), dp, out, gates, rows, K, H)
        ck = Ck(f"lstm ({K},{H}) rows {rows} ({'streamed' if rows < 2048 else 'weights-stationary'})",
                tiles=(rows, _waves(K, H, True)) if rows >= 2048 else None)
        ck.cmp("out", out[:2047].cpu(), r64["out"][:2047], r32["out"][:2047])
        ck.cmp("gates_save", gates[:2047].cpu(), r64["gates"][:2047], r32["gates"][:2047])
        ck.report()
        cks.append(ck)
    _finish(cks)


# ================================================================================================ B. Moebius head and linear
DIMS = (1, 3, 63, 64, 65, 127, 128, 129, 255, 256)
HEAD_ROWS = (1, 2, 3, 5, 39)


def _head(u, b_rows):
    return og.project(og.mobius_add(og.expmap0(u), b_rows), eps=4e-3)


def _head_case(g, rows, dim):
    """hypad_mobius_head_bwd with and without grad_bias_rows against autograd of project(mobius_add(expmap0(u), b)) with b expanded to
    one row per input row.  Tangent rows up to norm 3, one above 15 (the tanh clamp); the bias within radius 0.5: mobius_add with both
    operands near the rim has condition ~1 / (1 - |u|^2) in fp32 (tests/test_gpu_shape_sweep.py)."""
    c = _C()
    u = _ball_rows(g, rows, dim, tangent=True)
    b = _ball_rows(g, 1, dim, radius=0.5)[0]
    go = torch.randn(rows, dim, generator=g)
    res = {}
    for dt in (F64, F32):
        uu = _leaf(u, dt)
        bb = b.to(dt).unsqueeze(0).expand(rows, dim).clone().requires_grad_(True)
        res[dt] = torch.autograd.grad(_head(uu, bb), [uu, bb], go.to(dt))
    ud, bd, god = u.cuda(), b.cuda(), go.cuda()
    gu, gbr, gu2 = _nan(rows, dim), _nan(rows, dim), _nan(rows, dim)
    c.check(c.lib.hypad_mobius_head_bwd(c.ptr(ud), c.ptr(bd), c.ptr(god), c.ptr(gu), c.ptr(gbr), rows, dim, c.stream()), "mobius_head_bwd")
    c.check(c.lib.hypad_mobius_head_bwd(c.ptr(ud), c.ptr(bd), c.ptr(god), c.ptr(gu2), None, rows, dim, c.stream()), "mobius_head_bwd")
    ck = Ck(f"mobius_head_bwd dim {dim} rows {rows}")
    ck.cmp("grad_u", gu.cpu(), res[F64][0], res[F32][0])
    ck.cmp("grad_bias_rows", gbr.cpu(), res[F64][1], res[F32][1])
    ck.cmp("grad_u without grad_bias_rows", gu2.cpu(), res[F64][0], res[F32][0])
    return ck


@pytest.mark.parametrize("dim", DIMS)
def test_mobius_head_backward_every_layout(dim):
    g = torch.Generator().manual_seed(7000 + dim)
    cks = [_head_case(g, rows, dim) for rows in HEAD_ROWS]
    print(f"\ndense sweep mobius_head_bwd dim {dim}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")
    _finish(cks)


def test_mobius_head_backward_beyond_one_grid_stride():
    """70 001 rows at dim 65: more than the 16 384 rows one grid of head_rows_bwd covers (the rest grid-strides)."""
    ck = _head_case(torch.Generator().manual_seed(70001), 70001, 65)
    ck.report()
    _finish([ck])


def test_mobius_head_backward_refuses_dim_257():
    c = _C()
    a, gu, gb = torch.zeros(4, 257, device="cuda"), torch.full((4, 257), 7.0, device="cuda"), torch.full((4, 257), 7.0, device="cuda")
    assert c.lib.hypad_mobius_head_bwd(c.ptr(a), c.ptr(a), c.ptr(a), c.ptr(gu), c.ptr(gb), 4, 257, c.stream()) == HYPAD_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((gu == 7.0).all()) and bool((gb == 7.0).all())          # nothing ran


@pytest.mark.parametrize("rows,dim", [(0, 5), (1, 1), (39, 255), (39, 256), (39, 257), (4099, 300)])
def test_column_sum(rows, dim):
    c = _C()
    g = torch.Generator().manual_seed(rows + dim)
    a = torch.randn(rows, dim, generator=g)
    src = a.cuda() if rows else torch.zeros(1, device="cuda")            # (an empty tensor has no address)
    out = _nan(dim)
    c.check(c.lib.hypad_column_sum(c.ptr(src), c.ptr(out), rows, dim, c.stream()), "column_sum")
    ck = Ck(f"column_sum rows {rows} dim {dim}")
    ck.red("sum", out.cpu(), a.double().sum(0), a.double().abs().sum(0), rows)
    if rows == 0:
        assert bool((out == 0).all())
    ck.report()
    _finish([ck])


def _mobius_linear_ref(x, w, b_rows):
    """oracle.gmath.mobius_linear written out, so that the per-row pieces exist: u = x W^T is returned, the bias comes as one row per
    input row, and project takes the fp32 eps 4e-3 in fp64 too (og.mobius_linear lets project choose 1e-5 there: the row above the
    tanh clamp would land on another sphere than the kernel's)."""
    u = torch.nn.functional.linear(x, w)
    return og.project(og.mobius_add(og.expmap0(u), b_rows), eps=4e-3), u


def _mobius_linear_data(g, rows, K, N):
    """x ~ N(0, 1); weights scaled so that the largest |x W^T| is 2.5 (expmap0 stays off the rim: the conditioning note of _head_case),
    except row 1 (rows >= 3), stretched to norm 17: beyond the tanh clamp at 15."""
    x = torch.randn(rows, K, generator=g, dtype=F64)
    w = torch.randn(N, K, generator=g, dtype=F64)
    w = w * (2.5 / float((x @ w.t()).norm(dim=1).max()))
    if rows >= 3:
        x[1] *= 17.0 / float((x[1] @ w.t()).norm())
    b = _ball_rows(g, 1, N, radius=0.5)[0]
    return x.float(), w.float(), b, torch.randn(rows, N, generator=g)


def _mobius_linear_case(g, rows, K, N, unaligned=False):
    from hypad_amd.hyperspace import hyrnn_nets
    x, w, b, go = _mobius_linear_data(g, rows, K, N)
    res = {}
    for dt in (F64, F32):
        xx, ww = _leaf(x, dt), _leaf(w, dt)
        bb = b.to(dt).unsqueeze(0).expand(rows, N).clone().requires_grad_(True)
        o, u = _mobius_linear_ref(xx, ww, bb)
        gx, gw, gbr, gu = torch.autograd.grad(o, [xx, ww, bb, u], go.to(dt))
        res[dt] = dict(out=o.detach(), u=u.detach(), gx=gx, gw=gw, gbr=gbr, gu=gu)
    r64, r32 = res[F64], res[F32]
    mk = (lambda t: _unaligned(t.cuda())) if unaligned else (lambda t: t.cuda())
    xd, wd, bd = mk(x).requires_grad_(True), mk(w).requires_grad_(True), b.cuda().requires_grad_(True)
    out = hyrnn_nets.mobius_linear(xd, wd, bd, hyperbolic_input=False)
    u_saved = out.grad_fn.saved_tensors[3]
    out.backward(go.cuda())
    ck = Ck(f"mobius_linear ({K},{N}) rows {rows}{' unaligned' if unaligned else ''}")
    ck.cmp("out", out.detach().cpu(), r64["out"], r32["out"])
    ck.cmp("saved u", u_saved.cpu(), r64["u"], r32["u"])
    ck.cmp("grad_x", xd.grad.cpu(), r64["gx"], r32["gx"])
    x64 = x.double()
    ck.red("grad_weight", wd.grad.cpu(), r64["gw"], r64["gu"].abs().t() @ x64.abs(), rows,
           sc.grad_allowance(r64["gu"], r32["gu"]) * float(x64.abs().max()))
    ck.red("grad_bias", bd.grad.cpu(), r64["gbr"].sum(0), r64["gbr"].abs().sum(0), rows, sc.grad_allowance(r64["gbr"], r32["gbr"]))
    return ck


MOBIUS_KN = [(1, 1), (3, 5), (33, 63), (64, 64), (100, 100), (129, 65), (150, 150), (51, 256), (256, 256)]


@pytest.mark.parametrize("K,N", MOBIUS_KN)
def test_mobius_linear_forward_and_backward(K, N):
    g = torch.Generator().manual_seed(100 * K + N)
    cks = [_mobius_linear_case(g, rows, K, N) for rows in (1, 17, 39)]
    if (K, N) == (64, 64):
        cks.append(_mobius_linear_case(g, 39, K, N, unaligned=True))        # x and weight at storage offset 1
    print(f"\ndense sweep mobius_linear ({K},{N}): worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")
    _finish(cks)


def test_mobius_linear_refuses_width_257_and_a_short_workspace():
    c = _C()
    rows, K = 4, 8
    x, w257, b257 = torch.zeros(rows, K, device="cuda"), torch.zeros(257, K, device="cuda"), torch.zeros(257, device="cuda")
    out = torch.full((rows, 257), 7.0, device="cuda")
    assert c.lib.hypad_mobius_linear_fwd(c.ptr(x), c.ptr(w257), c.ptr(b257), c.ptr(out), None, rows, K, 257, c.stream()) == HYPAD_EUNSUPPORTED
    N = 16
    w, b, u, go = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda"), torch.zeros(rows, N, device="cuda"), torch.zeros(rows, N, device="cuda")
    gx, gw, gb = torch.full((rows, K), 7.0, device="cuda"), torch.full((N, K), 7.0, device="cuda"), torch.full((N,), 7.0, device="cuda")
    need = c.lib.hypad_mobius_linear_workspace_bytes(rows, N)
    assert need == rows * N * 2 * 4
    ws = torch.zeros(need // 4, device="cuda")
    args = lambda nbytes: (c.ptr(x), c.ptr(w), c.ptr(b), c.ptr(u), c.ptr(go), c.ptr(gx), c.ptr(gw), c.ptr(gb), c.ptr(ws), nbytes, rows, K, N, c.stream())
    assert c.lib.hypad_mobius_linear_bwd(*args(need - 4)) == HYPAD_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((gx == 7.0).all()) and bool((gw == 7.0).all()) and bool((gb == 7.0).all())      # nothing ran
    assert c.lib.hypad_mobius_linear_bwd(*args(need)) == 0


# ================================================================================================ C. linear and activation
ACTS = {"none": 0, "tanh": 1, "leaky": 2}           # HYPAD_ACT_*
# K through gemm_nt's weight-load forms (K % 4 == 0: 16-byte loads, K % 2 == 0: 8-byte, odd: scalar), one 32-k slab, one 128-k
# super-chunk and 257 -- each with an N that is and is not a multiple of 16; N through its column tiles -- each with a K of either kind
LINEAR_KN = ([(K, N) for K in (1, 2, 3, 4, 31, 32, 33, 34, 127, 128, 129, 130, 257) for N in (17, 64)]
             + [(K, N) for N in (1, 15, 16, 17, 63, 64, 65, 100, 257) for K in (33, 128)])


def _act(pre, act):
    if act == 1:
        return torch.tanh(pre)
    if act == 2:
        return torch.nn.functional.leaky_relu(pre, 0.2)
    return pre


def _linear_data(g, rows, K, N):
    return (torch.randn(rows, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, 0.1 * torch.randn(N, generator=g),
            torch.randn(rows, N, generator=g))


def _linear_refs(x, w, b, gy, act):
    res = {}
    for dt in (F64, F32):
        xx, ww, bb = (_leaf(t, dt) for t in (x, w, b))
        pre = torch.nn.functional.linear(xx, ww, bb)
        y = _act(pre, act)
        gx, gw, gb, gpre = torch.autograd.grad(y, [xx, ww, bb, pre], gy.to(dt))
        res[dt] = dict(y=y.detach(), gx=gx, gw=gw, gb=gb, gpre=gpre)
    return res


def _linear_reductions(ck, res, x, rows, gw, gb):
    r64, r32 = res[F64], res[F32]
    x64 = x.double()
    allow = sc.grad_allowance(r64["gpre"], r32["gpre"])
    if gw is not None:
        ck.red("grad_weight", gw.cpu(), r64["gw"], r64["gpre"].abs().t() @ x64.abs(), rows, allow * float(x64.abs().max()) if rows else 0.0)
    if gb is not None:
        ck.red("grad_bias", gb.cpu(), r64["gb"], r64["gpre"].abs().sum(0), rows, allow)


def _linear_direct(ck, x, w, b, gy, act, w_dev=None, forms=("full",)):
    """hypad_linear_act_fwd and _bwd called directly (the backward on the GPU's own y)."""
    c = _C()
    rows, K, N = x.shape[0], x.shape[1], w.shape[0]
    res = _linear_refs(x, w, b, gy, act)
    r64, r32 = res[F64], res[F32]
    xd, wd, bd, gyd = x.cuda(), (w.cuda() if w_dev is None else w_dev), b.cuda(), gy.cuda()
    y = _nan(rows, N)
    c.check(c.lib.hypad_linear_act_fwd(c.ptr(xd), c.ptr(wd), c.ptr(bd), c.ptr(y), rows, K, N, act, c.stream()), "linear_act_fwd")
    ck.cmp("y", y.cpu(), r64["y"], r32["y"])
    for form in forms:
        want = dict(full=("gx", "gw", "gb", "gpre"), no_gx=("gw", "gb", "gpre"), no_gb=("gx", "gw", "gpre"), gpre_only=("gpre",))[form]
        o = dict(gx=_nan(rows, K), gw=_nan(N, K), gb=_nan(N), gpre=_nan(rows, N))
        p = lambda k: c.ptr(o[k]) if k in want else None
        c.check(c.lib.hypad_linear_act_bwd(c.ptr(xd), c.ptr(wd), c.ptr(y), c.ptr(gyd), p("gx"), p("gw"), p("gb"), p("gpre"), rows, K, N, act,
                                           c.stream()), f"linear_act_bwd {form}")
        tag = "" if form == "full" else f" [{form}]"
        if "gx" in want:
            ck.cmp("grad_x" + tag, o["gx"].cpu(), r64["gx"], r32["gx"])
        ck.cmp("grad_pre" + tag, o["gpre"].cpu(), r64["gpre"], r32["gpre"])
        _linear_reductions(ck, res, x, rows, o["gw"] if "gw" in want else None, o["gb"] if "gb" in want else None)
        for k in o:
            if k not in want:
                assert bool(torch.isnan(o[k]).all()), (form, k)          # (not asked for: not written)
    return res


def _linear_autograd(ck, x, w, b, gy, act, res):
    from hypad_amd import autograd as hag
    rows = x.shape[0]
    xd, wd, bd = (t.cuda().requires_grad_(True) for t in (x, w, b))
    y = hag.linear_act(xd, wd, bd, act)
    y.backward(gy.cuda())
    r64, r32 = res[F64], res[F32]
    ck.cmp("autograd y", y.detach().cpu(), r64["y"], r32["y"])
    ck.cmp("autograd x.grad", xd.grad.cpu(), r64["gx"], r32["gx"])
    _linear_reductions(ck, res, x, rows, wd.grad, bd.grad)


@pytest.mark.parametrize("act", list(ACTS))
def test_linear_act_at_the_edges_of_its_tiles(act):
    g = torch.Generator().manual_seed(31 + ACTS[act])
    cks = []
    for K, N in LINEAR_KN:
        x, w, b, gy = _linear_data(g, 39, K, N)
        ck = Ck(f"linear_act {act} ({K},{N}) rows 39")
        res = _linear_direct(ck, x, w, b, gy, ACTS[act])
        _linear_autograd(ck, x, w, b, gy, ACTS[act], res)
        cks.append(ck)
    print(f"\ndense sweep linear_act {act}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f}")
    _finish(cks)


@pytest.mark.parametrize("rows", (1, 3, 4, 5, 15, 16, 17, 39, 4099))
def test_linear_act_row_counts(rows):
    """(100, 77) with tanh: outer_sum_kernel's four-row steps with one to three rows left over, one and many 16-row tiles."""
    g = torch.Generator().manual_seed(rows)
    x, w, b, gy = _linear_data(g, rows, 100, 77)
    ck = Ck(f"linear_act tanh (100,77) rows {rows}")
    res = _linear_direct(ck, x, w, b, gy, 1)
    _linear_autograd(ck, x, w, b, gy, 1, res)
    ck.report()
    _finish([ck])


@pytest.mark.parametrize("K", (128, 130))
@pytest.mark.parametrize("offset", (1, 2))
def test_linear_act_weight_pointer_offsets(K, offset):
    """The weight matrix at storage offset 1 (4-byte aligned: scalar weight loads) and 2 (8-byte aligned: 8-byte loads) of a shape
    that takes 16-byte (K = 128) or 8-byte (K = 130) loads when aligned."""
    g = torch.Generator().manual_seed(10 * K + offset)
    x, w, b, gy = _linear_data(g, 39, K, 64)
    ck = Ck(f"linear_act tanh ({K},64) rows 39, weight at offset {offset}")
    _linear_direct(ck, x, w, b, gy, 1, w_dev=_at_offset(w.cuda(), offset))
    ck.report()
    _finish([ck])


def test_linear_act_backward_partial_forms():
    """grad_x = NULL; grad_weight without grad_bias; grad_pre only."""
    g = torch.Generator().manual_seed(5)
    x, w, b, gy = _linear_data(g, 39, 33, 17)
    ck = Ck("linear_act leaky (33,17) rows 39")
    _linear_direct(ck, x, w, b, gy, 2, forms=("no_gx", "no_gb", "gpre_only"))
    ck.report()
    _finish([ck])


# ================================================================================================ D. argument checks and the empty batch
def test_linear_act_backward_refuses_a_bias_gradient_without_a_weight_gradient_before_it_writes():
    c = _C()
    rows, K, N = 39, 33, 17
    x, w, y, gy = (torch.zeros(s, device="cuda") for s in ((rows, K), (N, K), (rows, N), (rows, N)))
    gx, gpre, gb = torch.full((rows, K), SENTINEL, device="cuda"), torch.full((rows, N), SENTINEL, device="cuda"), torch.full((N,), SENTINEL, device="cuda")
    rc = c.lib.hypad_linear_act_bwd(c.ptr(x), c.ptr(w), c.ptr(y), c.ptr(gy), c.ptr(gx), None, c.ptr(gb), c.ptr(gpre), rows, K, N, 1, c.stream())
    torch.cuda.synchronize()
    assert rc == HYPAD_EINVAL
    assert bool((gx == SENTINEL).all()) and bool((gpre == SENTINEL).all()) and bool((gb == SENTINEL).all())


def _poison(*shapes):
    """Leave NaN in the allocator's free blocks of these sizes: the next torch.empty of such a size gets them back."""
    ts = [torch.full(tuple(s), NAN, device="cuda") for s in shapes]
    torch.cuda.synchronize()
    del ts


def _all_zero_grads(params):
    for n, p in params:
        assert p.grad is not None and p.grad.shape == p.shape and bool((p.grad == 0).all()), n


def test_empty_batch_through_linear_act_leaves_zero_parameter_gradients():
    from hypad_amd import autograd as hag
    lin = torch.nn.Linear(33, 17).cuda()
    x = torch.empty(0, 33, device="cuda", requires_grad=True)
    y = hag.linear_act(x, lin.weight, lin.bias, 1)
    assert y.shape == (0, 17)
    _poison(lin.weight.shape, lin.bias.shape)
    y.sum().backward()
    _all_zero_grads(lin.named_parameters())
    assert x.grad.shape == (0, 33)


def test_empty_batch_through_lstm_layer_leaves_zero_parameter_gradients():
    from hypad_amd import autograd as hag
    lstm = torch.nn.LSTM(100, 50, bidirectional=True).cuda()
    x = torch.empty(0, 100, device="cuda", requires_grad=True)
    out = hag.lstm_layer(x, lstm, 0)
    assert out.shape == (0, 100)
    _poison(*[p.shape for p in lstm.parameters()])
    out.sum().backward()
    _all_zero_grads(lstm.named_parameters())
    assert x.grad.shape == (0, 100)


def test_empty_batch_through_mobius_linear_leaves_zero_parameter_gradients():
    from hypad_amd.hyperspace import hyrnn_nets
    w = torch.randn(17, 33, device="cuda", requires_grad=True)
    b = (0.01 * torch.randn(17, device="cuda")).requires_grad_(True)
    x = torch.empty(0, 33, device="cuda", requires_grad=True)
    out = hyrnn_nets.mobius_linear(x, w, b, hyperbolic_input=False)
    assert out.shape == (0, 17)
    _poison(w.shape, b.shape)
    out.sum().backward()
    _all_zero_grads([("weight", w), ("bias", b)])
    assert x.grad.shape == (0, 33)
