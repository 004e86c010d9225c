"""The general-T bidirectional LSTM layer (csrc/lstm_seq.hip: hypad_lstm_bidir_seq_fwd, _fwd_train, _bwd; hypad_amd.autograd.lstm_seq)
against a plain fp64 time loop on the CPU (tests/lstm_seq_ref.py, itself pinned to fp64 torch.nn.LSTM by
tests/test_lstm_seq_reference.py): every padded hidden size HP in {16, 32, 48, 64} at both of its edges, row counts around the 16-row
tile, sequence lengths 1 .. 5, 64 and 100, every NULL-argument form of the C ABI, guard floats and 4-byte-aligned buffers, gates
driven past fp32 exp's range, tile independence and the empty batch.

Two rules, both from sweep_common (``Ck``).

Per-row quantities (out, h_n, c_n, saved, grad_x, grad_h0, grad_c0) go under ``Checker.cmp``: errgpu <= C * err32 + T * F with that
file's C = 8 and F = 2e-6, err32 being the error of the same loop run in fp32 on the CPU.  The floor is T * F for a sequence of T
steps: F is what one application of the device activations (hardware exp and reciprocal) was given at T = 1, a recurrence applies
them T times, and err32 already carries the growth of rounding.  T = 1 is the rule unchanged.

The parameter gradients (grad_w_ih, grad_w_hh, grad_b of both directions) are sums over T * rows terms and go under the reduction
rule ``Ck.red`` with rows := T * rows: the summands are the pre-activation gradients times x, h_prev or 1; their allowance is
``grad_allowance`` of the reference's fp64 and fp32 pre-activation gradients times the largest |x|, |h_prev| or 1.
"""
import pytest
import torch

import lstm_seq_ref as lr
import sweep_common as sc
from sweep_common import NAN, Ck, _at_offset, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_OK, HYPAD_EINVAL = 0, -1                       # include/hypad.h
ALL = (True, True, True)


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks, what):
    print(f"\nlstm_seq sweep {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}, "
          f"worst reduction error / allowance {max(ck.rworst for ck in cks):.3f} over {len(cks)} cases")
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ data and reference
def _data(T, rows, K, H, seed=0, bias_hh=None):
    """x ~ N(0, 1); h0, c0 ~ 0.5 N(0, 1); the eight parameters at torch's default initialisation U(-1/sqrt(H), 1/sqrt(H)); upstream
    gradients ~ N(0, 1) for out, h_n and c_n.  All float32 on the CPU."""
    g = torch.Generator().manual_seed(100003 * T + 1009 * rows + 101 * K + H + seed)
    bound = 1.0 / H ** 0.5
    shapes = [(4 * H, K), (4 * H, H), (4 * H,), (4 * H,)] * 2
    params = [(torch.rand(*s, generator=g) * 2 - 1) * bound for s in shapes]
    if bias_hh is not None:
        params[3], params[7] = bias_hh[0].clone(), bias_hh[1].clone()
    return dict(T=T, rows=rows, K=K, H=H, params=params, x=torch.randn(T, rows, K, generator=g),
                h0=0.5 * torch.randn(2, rows, H, generator=g), c0=0.5 * torch.randn(2, rows, H, generator=g),
                up=[torch.randn(T, rows, 2 * H, generator=g), torch.randn(2, rows, H, generator=g), torch.randn(2, rows, H, generator=g)])


def _ref(d, use_h0=True, use_c0=True, up=ALL):
    """{F64: ..., F32: ...}: lstm_seq_ref.run with the states and upstream gradients that are asked for."""
    ups = [u if on else None for u, on in zip(d["up"], up)]
    return {dt: lr.run(d["x"], d["params"], d["h0"] if use_h0 else None, d["c0"] if use_c0 else None, *ups, dtype=dt) for dt in (F64, F32)}


def _cmp_forward(ck, d, ref, got, keys=("out", "hn", "cn", "saved")):
    r64, r32 = ref[F64], ref[F32]
    for k in keys:
        if got.get(k) is not None:
            ck.cmp(k, got[k], r64[k], r32[k], steps=d["T"])


def _cmp_backward(ck, d, ref, got):
    """got: gx, gh0 / gc0 (or None), gw_ih, gw_hh, gb: pairs (forward, reverse)."""
    r64, r32 = ref[F64], ref[F32]
    T, rows = d["T"], d["rows"]
    ck.cmp("grad_x", got["gx"], r64["gx"], r32["gx"], steps=T)
    for k in ("gh0", "gc0"):
        if got.get(k) is not None:
            ck.cmp("grad_" + k[1:], got[k], r64[k], r32[k], steps=T)
    x64 = d["x"].double().reshape(T * rows, -1)
    for dr, tag in enumerate(("forward", "reverse")):
        a64 = r64["dpre"][dr].reshape(T * rows, -1)
        allow = sc.grad_allowance(r64["dpre"][dr], r32["dpre"][dr])
        hp = r64["hprev"][dr].reshape(T * rows, -1)
        ck.red(f"grad weight_ih {tag}", got["gw_ih"][dr], r64["gp"][4 * dr], a64.abs().t() @ x64.abs(), T * rows, allow * float(x64.abs().max()))
        ck.red(f"grad weight_hh {tag}", got["gw_hh"][dr], r64["gp"][4 * dr + 1], a64.abs().t() @ hp.abs(), T * rows, allow * float(hp.abs().max()))
        ck.red(f"grad bias {tag}", got["gb"][dr], r64["gp"][4 * dr + 2], a64.abs().sum(0), T * rows, allow)


# ------------------------------------------------------------------------------------------------ the two ways to the kernels
def _abi(d, use_h0=True, use_c0=True, up=ALL, offset=16, want=("hn", "cn", "saved", "gh0", "gc0"), train=True):
    """The C ABI called directly.  Every output is a NaN-filled view with a sentinel float on both sides, at storage offset ``offset``
    floats (16: 64-byte aligned; 1: 4-byte aligned only, and then x, the states and the upstream gradients sit at offset 1 too).  An
    output that is not in ``want`` (or whose state is not given) is passed as NULL.  Returns the results on the CPU plus 'guards'
    (names of outputs whose sentinels were overwritten) and 'nan' (names of outputs that kept a NaN)."""
    c = _C()
    T, rows, K, H = d["T"], d["rows"], d["K"], d["H"]
    dev = (lambda t: _at_offset(t.cuda(), 1)) if offset == 1 else (lambda t: t.cuda())
    x, ps = dev(d["x"]), [p.cuda() for p in d["params"]]
    h0 = dev(d["h0"]) if use_h0 else None
    c0 = dev(d["c0"]) if use_c0 else None
    bufs = {}

    def out(name, shape, on=True):
        if not on:
            return None
        bufs[name] = _guarded(shape, offset)
        return bufs[name][1]
    o, hn, cn = out("out", (T, rows, 2 * H)), out("hn", (2, rows, H), "hn" in want), out("cn", (2, rows, H), "cn" in want)
    saved = out("saved", (T, rows, 2, 5, H), train and "saved" in want)
    nbytes = c.lib.hypad_lstm_seq_workspace_bytes(T, rows, H)
    ws = torch.empty(max(nbytes // 4, 1), device="cuda")
    if train:
        c.check(c.lib.hypad_lstm_bidir_seq_fwd_train(c.ptr(x), *[c.ptr(p) for p in ps], c.ptr(h0), c.ptr(c0), c.ptr(o), c.ptr(hn), c.ptr(cn), c.ptr(saved),
                                                     T, rows, K, H, ws.data_ptr(), nbytes, c.stream()), "lstm_bidir_seq_fwd_train")
    else:
        c.check(c.lib.hypad_lstm_bidir_seq_fwd(c.ptr(x), *[c.ptr(p) for p in ps], c.ptr(h0), c.ptr(c0), c.ptr(o), c.ptr(hn), c.ptr(cn),
                                               T, rows, K, H, ws.data_ptr(), nbytes, c.stream()), "lstm_bidir_seq_fwd")
    if saved is not None and any(up):
        gup = [dev(u) if on else None for u, on in zip(d["up"], up)]
        gx = out("gx", (T, rows, K))
        gp = [out(n, s) for n, s in (("gw_ih_f", (4 * H, K)), ("gw_hh_f", (4 * H, H)), ("gb_f", (4 * H,)),
                                     ("gw_ih_r", (4 * H, K)), ("gw_hh_r", (4 * H, H)), ("gb_r", (4 * H,)))]
        gh0, gc0 = out("gh0", (2, rows, H), use_h0 and "gh0" in want), out("gc0", (2, rows, H), use_c0 and "gc0" in want)
        nb = c.lib.hypad_lstm_seq_bwd_workspace_bytes(T, rows, K, H)
        ws2 = torch.empty(max(nb // 4, 1), device="cuda")
        c.check(c.lib.hypad_lstm_bidir_seq_bwd(c.ptr(x), c.ptr(ps[0]), c.ptr(ps[1]), c.ptr(ps[4]), c.ptr(ps[5]), c.ptr(h0), c.ptr(c0), c.ptr(o), c.ptr(saved),
                                               *[c.ptr(g) for g in gup], c.ptr(gx), *[c.ptr(g) for g in gp], c.ptr(gh0), c.ptr(gc0), T, rows, K, H,
                                               ws2.data_ptr(), nb, c.stream()), "lstm_bidir_seq_bwd")
    torch.cuda.synchronize()
    got = {k: v.cpu() for k, (_, v) in bufs.items()}
    got["guards"] = [k for k, (b, _) in bufs.items() if not _guards_intact(b, offset)]
    got["nan"] = [k for k, v in got.items() if isinstance(v, torch.Tensor) and bool(torch.isnan(v).any())]
    if "gx" in got:
        got.update(gw_ih=(got["gw_ih_f"], got["gw_ih_r"]), gw_hh=(got["gw_hh_f"], got["gw_hh_r"]), gb=(got["gb_f"], got["gb_r"]))
    return got


def _clean(ck, got):
    if got["guards"]:
        ck.failures.append(f"{ck.case}: a guard float next to {got['guards']} was overwritten")
    if got["nan"]:
        ck.failures.append(f"{ck.case}: {got['nan']} kept a NaN (an element was not written)")


def _module(d):
    lstm = torch.nn.LSTM(d["K"], d["H"], num_layers=1, bidirectional=True)
    with torch.no_grad():
        for n, p in zip(lr.PARAM_NAMES, d["params"]):
            getattr(lstm, n).copy_(p)
    return lstm.cuda()


def _autograd(d, with_state=True, up=ALL):
    """hypad_amd.autograd.lstm_seq; bias_ih and bias_hh must receive the same gradient."""
    from hypad_amd import autograd as hag
    lstm = _module(d)
    x = d["x"].cuda().requires_grad_(True)
    hx = (d["h0"].cuda().requires_grad_(True), d["c0"].cuda().requires_grad_(True)) if with_state else None
    out, (hn, cn) = hag.lstm_seq(x, lstm, 0, hx)
    loss = sum((o * u.cuda()).sum() for o, u, on in zip((out, hn, cn), d["up"], up) if on)
    loss.backward()
    torch.cuda.synchronize()
    g = lambda n: getattr(lstm, n).grad.cpu()
    assert torch.equal(g("bias_ih_l0"), g("bias_hh_l0")) and torch.equal(g("bias_ih_l0_reverse"), g("bias_hh_l0_reverse"))
    return dict(out=out.detach().cpu(), hn=hn.detach().cpu(), cn=cn.detach().cpu(), gx=x.grad.cpu(),
                gh0=hx[0].grad.cpu() if with_state else None, gc0=hx[1].grad.cpu() if with_state else None,
                gw_ih=(g("weight_ih_l0"), g("weight_ih_l0_reverse")), gw_hh=(g("weight_hh_l0"), g("weight_hh_l0_reverse")),
                gb=(g("bias_ih_l0"), g("bias_ih_l0_reverse")))


def _autograd_case(T, rows, K, H, with_state):
    d = _data(T, rows, K, H)
    ref = _ref(d, with_state, with_state)
    ck = Ck(f"autograd.lstm_seq T {T} rows {rows} K {K} H {H}{' with states' if with_state else ''}")
    got = _autograd(d, with_state)
    _cmp_forward(ck, d, ref, got, ("out", "hn", "cn"))
    _cmp_backward(ck, d, ref, got)
    return ck


def _abi_case(T, rows, K, H, with_state=True, offset=16, d=None, tag=""):
    d = d or _data(T, rows, K, H)
    ref = _ref(d, with_state, with_state)
    ck = Ck(f"C ABI T {T} rows {rows} K {K} H {H}{' with states' if with_state else ''}{tag}")
    got = _abi(d, with_state, with_state, offset=offset)
    _clean(ck, got)
    _cmp_forward(ck, d, ref, got)
    _cmp_backward(ck, d, ref, got)
    return ck, got


# ================================================================================================ 1. every HP class at both edges
def test_every_padded_hidden_size_at_both_edges():
    """H in {1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64} at T = 3 (both halves of the double-buffered LDS tiles; the last step
    writes the half the first one read), 21 rows (one full tile and one of 5 rows), K = 9, with and without initial states, upstream
    gradients on all three outputs.  Through the C ABI, so that `saved` is compared too."""
    cks = [_abi_case(3, 21, 9, H, ws)[0] for H in (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64) for ws in (True, False)]
    _finish(cks, "HP edges")


# ================================================================================================ 2. row edges
def test_row_counts_around_the_tile_and_many_workgroups():
    cks = [_autograd_case(T, rows, 12, 20, rows % 2 == 1) for rows in (1, 15, 16, 17, 32, 33) for T in (1, 2)]
    cks += [_abi_case(T, rows, 12, 20, rows % 2 == 0)[0] for rows in (1, 15, 16, 17, 32, 33) for T in (1, 2)]
    cks.append(_autograd_case(2, 2083, 50, 50, True))                      # 131 workgroups per direction
    _finish(cks, "row edges")


# ================================================================================================ 3. sequence lengths
def test_sequence_lengths_one_to_five():
    cks = [_abi_case(T, 17, 12, 33, ws)[0] for T in (1, 2, 3, 4, 5) for ws in (True, False)]
    cks += [_autograd_case(T, 17, 12, 33, True) for T in (1, 2, 3, 4, 5)]
    _finish(cks, "T 1..5")


@pytest.mark.parametrize("T,rows,K,H", [(64, 33, 20, 32), (100, 16, 7, 64)])
def test_long_sequences(T, rows, K, H):
    cks = [_abi_case(T, rows, K, H, True)[0], _autograd_case(T, rows, K, H, False)]
    _finish(cks, f"T {T}")


# ================================================================================================ 4. the ABI's optional arguments
def test_optional_arguments_of_the_c_abi():
    """(T 4, 19 rows, K 10, H 20).  Forward: h0 only, c0 only, hn NULL, cn NULL, saved NULL (the inference entry point: same bits in
    out / hn / cn as the training form).  Backward: each single upstream gradient and each pair; grad_h0 and / or grad_c0 NULL.  The
    reference omits the corresponding term each time; an output that is not asked for is NULL, every other one is guarded."""
    T, rows, K, H = 4, 19, 10, 20
    d = _data(T, rows, K, H)
    cks = []
    full = _abi(d)
    for use_h0, use_c0 in ((True, False), (False, True)):
        ck = Ck(f"{'h0' if use_h0 else 'c0'} only")
        ref = _ref(d, use_h0, use_c0)
        got = _abi(d, use_h0, use_c0)
        assert ("gh0" in got) == use_h0 and ("gc0" in got) == use_c0
        _clean(ck, got); _cmp_forward(ck, d, ref, got); _cmp_backward(ck, d, ref, got)
        cks.append(ck)
    ref = _ref(d)
    for missing in ("hn", "cn"):
        ck = Ck(f"{missing} NULL")
        got = _abi(d, want=tuple(k for k in ("hn", "cn", "saved", "gh0", "gc0") if k != missing))
        assert missing not in got
        _clean(ck, got); _cmp_forward(ck, d, ref, got); _cmp_backward(ck, d, ref, got)
        for k in ("out", "hn", "cn", "saved", "gx"):
            if k != missing and not torch.equal(got[k], full[k]):
                ck.failures.append(f"{ck.case}: {k} differs in bits from the call with every output")
        cks.append(ck)
    ck = Ck("saved NULL (hypad_lstm_bidir_seq_fwd)")
    got = _abi(d, train=False)
    assert "saved" not in got and "gx" not in got
    _clean(ck, got); _cmp_forward(ck, d, ref, got)
    for k in ("out", "hn", "cn"):
        if not torch.equal(got[k], full[k]):
            ck.failures.append(f"{ck.case}: {k} differs in bits from the training form")
    cks.append(ck)
    for up in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
        names = " + ".join(n for n, on in zip(("grad_out", "grad_hn", "grad_cn"), up) if on)
        ck = Ck(f"upstream {names} only")
        got = _abi(d, up=up)
        _clean(ck, got); _cmp_backward(ck, d, _ref(d, up=up), got)
        cks.append(ck)
    for want in (("gh0",), ("gc0",), ()):
        ck = Ck(f"grad_h0 / grad_c0: only {want or 'neither'}")
        got = _abi(d, want=("hn", "cn", "saved") + want)
        assert ("gh0" in got) == ("gh0" in want) and ("gc0" in got) == ("gc0" in want)
        _clean(ck, got); _cmp_backward(ck, d, ref, got)
        for k in ("gx", "gw_hh_r", "gb_f") + want:
            if not torch.equal(got[k], full[k]):
                ck.failures.append(f"{ck.case}: {k} differs in bits from the call with both state gradients")
        cks.append(ck)
    _finish(cks, "optional arguments")


# ================================================================================================ 5. guards and alignment
@pytest.mark.parametrize("T,rows,K,H", [(3, 21, 9, 33), (2, 17, 128, 64)])
def test_guard_floats_and_four_byte_aligned_buffers(T, rows, K, H):
    """Every output of forward and backward is a NaN-filled view between two sentinel floats; once 64-byte aligned, once with x, the
    states, out, saved, the upstream gradients and all gradient buffers at storage offset 1.  Both obey the rules; sentinels intact; no
    NaN left."""
    d = _data(T, rows, K, H)
    (ck_a, a), (ck_m, m) = _abi_case(T, rows, K, H, True, 16, d, " aligned"), _abi_case(T, rows, K, H, True, 1, d, " at offset 1")
    assert set(a) == set(m) and {"out", "hn", "cn", "saved", "gx", "gh0", "gc0", "gw_ih_f", "gw_hh_f", "gb_f", "gw_ih_r", "gw_hh_r", "gb_r"} <= set(a)
    _finish([ck_a, ck_m], f"guards T {T} H {H}")


# ================================================================================================ 6. saturated gates
def test_gates_beyond_the_range_of_fp32_exp():
    """(T 3, 16 rows, K 4, H 16).  bias_hh puts the pre-activations of i, f, g and o of unit u near +-30, +-100 or +-200 (u % 3), the
    sign of gate k from bit k of u: every sign pattern of the four gates, each magnitude five times.  +-100 and +-200 are beyond fp32
    exp's range (e^88.7 = FLT_MAX): the device sigmoid and tanh then rest on rcp(inf) = 0.  Everything finite and within the rules."""
    T, rows, K, H = 3, 16, 4, 16
    b = torch.zeros(2, 4 * H)
    for u in range(H):
        for k in range(4):
            b[:, k * H + u] = (30.0, 100.0, 200.0)[u % 3] * (1.0 if (u >> k) & 1 else -1.0)
    b[1] = -b[1]
    d = _data(T, rows, K, H, bias_hh=b)
    sv = _ref(d)[F64]["saved"]
    assert float(sv[..., 0, :].min()) < 1e-12 and float(sv[..., 0, :].max()) > 1 - 1e-12      # (the gates really are saturated)
    ck, got = _abi_case(T, rows, K, H, True, d=d, tag=" saturated")
    ck2 = Ck("autograd.lstm_seq saturated")
    got2 = _autograd(d)
    _cmp_forward(ck2, d, _ref(d), got2, ("out", "hn", "cn")); _cmp_backward(ck2, d, _ref(d), got2)
    for g_, c_ in ((got, ck), (got2, ck2)):
        for k, v in g_.items():
            for t in (v if isinstance(v, tuple) else (v,)):
                if isinstance(t, torch.Tensor) and not bool(torch.isfinite(t).all()):
                    c_.failures.append(f"{c_.case}: {k} is not finite")
    _finish([ck, ck2], "saturated gates")


# ================================================================================================ 7. tile independence
def test_rows_do_not_depend_on_their_tile():
    """Rows 3 .. 7 of a 40-row batch, run as a 5-row batch of their own, give the same bits in out, h_n, c_n and grad_x."""
    T, K, H = 3, 12, 33
    d = _data(T, 40, K, H)
    s = dict(d, rows=5, x=d["x"][:, 3:8].contiguous(), h0=d["h0"][:, 3:8].contiguous(), c0=d["c0"][:, 3:8].contiguous(),
             up=[d["up"][0][:, 3:8].contiguous(), d["up"][1][:, 3:8].contiguous(), d["up"][2][:, 3:8].contiguous()])
    big, small = _abi(d), _abi(s)
    ck = Ck("rows 3..7 of 40 as a batch of 5")
    _clean(ck, big); _clean(ck, small)
    _cmp_forward(ck, s, _ref(s), small)
    for k, sl in (("out", big["out"][:, 3:8]), ("hn", big["hn"][:, 3:8]), ("cn", big["cn"][:, 3:8]), ("gx", big["gx"][:, 3:8])):
        if not torch.equal(small[k], sl):
            ck.failures.append(f"{ck.case}: {k} differs in bits, max |diff| {float((small[k] - sl).abs().max()):.3e}")
    _finish([ck], "tile independence")


# ================================================================================================ 8. the empty batch
def test_empty_batch():
    """rows == 0 returns HYPAD_OK from all three entry points with NULL row buffers and a NULL workspace; the backward writes exact
    zeros to the six parameter gradients (and to nothing else); seq_len <= 0 stays HYPAD_EINVAL.  autograd.lstm_seq and
    lstm_seq_forward take an empty batch like lstm_layer and linear_act do."""
    from hypad_amd import autograd as hag
    c = _C()
    T, K, H = 3, 12, 20
    d = _data(T, 1, K, H)
    ps = [p.cuda() for p in d["params"]]
    pp = [c.ptr(p) for p in ps]
    s = c.stream()
    assert c.lib.hypad_lstm_seq_workspace_bytes(T, 0, H) == 0 and c.lib.hypad_lstm_seq_bwd_workspace_bytes(T, 0, K, H) == 0
    assert c.lib.hypad_lstm_bidir_seq_fwd(None, *pp, None, None, None, None, None, T, 0, K, H, None, 0, s) == HYPAD_OK
    assert c.lib.hypad_lstm_bidir_seq_fwd_train(None, *pp, None, None, None, None, None, None, T, 0, K, H, None, 0, s) == HYPAD_OK
    shapes = [(4 * H, K), (4 * H, H), (4 * H,)] * 2
    bufs = [_guarded(sh, 16) for sh in shapes]
    w4 = [pp[0], pp[1], pp[4], pp[5]]
    bwd = lambda T_: c.lib.hypad_lstm_bidir_seq_bwd(None, *w4, None, None, None, None, None, None, None, None, *[c.ptr(v) for _, v in bufs], None, None,
                                                   T_, 0, K, H, None, 0, s)
    assert bwd(0) == HYPAD_EINVAL and bwd(-1) == HYPAD_EINVAL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for _, v in bufs)                  # (refused: nothing written)
    assert bwd(T) == HYPAD_OK
    torch.cuda.synchronize()
    assert all(bool((v == 0).all()) and _guards_intact(b, 16) for b, v in bufs)
    for T_ in (0, -1):
        assert c.lib.hypad_lstm_bidir_seq_fwd(None, *pp, None, None, None, None, None, T_, 0, K, H, None, 0, s) == HYPAD_EINVAL
        assert c.lib.hypad_lstm_bidir_seq_fwd_train(None, *pp, None, None, None, None, None, None, T_, 0, K, H, None, 0, s) == HYPAD_EINVAL
    for with_state in (False, True):
        lstm = _module(d)
        x = torch.empty(T, 0, K, device="cuda", requires_grad=True)
        hx = (torch.empty(2, 0, H, device="cuda", requires_grad=True), torch.empty(2, 0, H, device="cuda", requires_grad=True)) if with_state else None
        out, (hn, cn) = hag.lstm_seq(x, lstm, 0, hx)
        assert out.shape == (T, 0, 2 * H) and hn.shape == (2, 0, H) and cn.shape == (2, 0, H)
        junk = [torch.full(tuple(p.shape), NAN, device="cuda") for p in lstm.parameters()]      # NaN into the allocator's free blocks of these sizes
        torch.cuda.synchronize()
        del junk
        (out.sum() + hn.sum() + cn.sum()).backward()
        for n, p in lstm.named_parameters():
            assert p.grad is not None and p.grad.shape == p.shape and bool((p.grad == 0).all()), n
        assert x.grad.shape == (T, 0, K) and (not with_state or hx[0].grad.shape == (2, 0, H))
        with torch.no_grad():
            o2, (h2, c2) = hag.lstm_seq_forward(x.detach(), lstm, 0, None if hx is None else (hx[0].detach(), hx[1].detach()))
        assert o2.shape == (T, 0, 2 * H) and h2.shape == (2, 0, H) and c2.shape == (2, 0, H)
