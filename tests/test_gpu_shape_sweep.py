"""Runtime-shape builds against fp64 oracle/manual.py under the rule of tests/sweep_common.py (errgpu <= C * err32 + F).

Every shape but the two anchors runs the <0,0,0> (runtime-shape) instantiations of the training and scoring kernels: one iteration of
each kind with every gradient, moment and updated parameter (ball bias included), the captured epoch teacher-forced on its full
optimizer state, the scoring forward at every row-layout class with partial tiles, and the stand-alone Poincare-ball kernels at every
row layout, the unaligned fallback and the grid-stride tail."""
import ctypes

import numpy as np
import pytest
import torch

import sweep_common as sc
from sweep_common import _ball_rows, _unaligned
from epoch_oracle import NB, NC, cu
from epoch_oracle import check_step as _check_step, engine as _engine, epoch_against_oracle as _epoch_against_oracle, state as _state
from oracle import gmath as og
from oracle import manual

pytestmark = pytest.mark.gpu

F64 = torch.float64
HYPAD_EUNSUPPORTED = -3          # include/hypad.h



WORST = {}


def _one_of_each(S, L, B, hyper, tag, masks=None):
    sd32 = sc.init_state(S, L, hyper)
    sd64 = sc.cast(sd32, F64)
    x, z, ax, az = sc.iteration_data(S, L, B)
    eng = _engine(S, L, B, hyper, [sd32])
    xs = x.cuda().view(1, B, S)
    train = masks is not None
    fl = (lambda *ts: torch.cat([t.reshape(-1) for t in ts]).cuda()) if train else None
    lx = eng.critic_x_iteration(xs, None, z.cuda(), ax.cuda(), train_mode=train,
                                masks=fl(*masks["cx"]["valid"], *masks["cx"]["fake"], *masks["cx"]["inter"], masks["cx"]["dec"]) if train else None)
    lz = eng.critic_z_iteration(xs, None, z.cuda(), az.cuda(), train_mode=train,
                                masks=fl(*masks["cz"]["fake"], *masks["cz"]["valid"], *masks["cz"]["inter"]) if train else None)
    after_c = _state(eng, ("cx", "cz"))
    critics = {k: v for k, v in after_c[0].items()}            # the critics just moved: the generator step is compared at them
    ld = eng.decoder_iteration(xs, None, z.cuda(), train_mode=train,
                               masks=fl(*masks["dec"]["cz"], *masks["dec"]["cx"], masks["dec"]["dec_gen"], masks["dec"]["dec_rec"]) if train else None)
    torch.cuda.synchronize()
    after_g = _state(eng, ("dec", "enc"))
    r64 = sc.iterations(sd64, x, z, ax, az, hyper, masks, critics_after=critics)
    r32 = sc.iterations(sd32, x, z, ax, az, hyper, masks, critics_after=critics)
    ck = sc.Checker(f"{'hyper' if hyper else 'eucl'} ({S},{L},{B}){' train' if train else ''}")
    ck.cmp("critic_x loss", lx[0, 0].cpu(), r64["cx"][0], r32["cx"][0])
    ck.cmp("critic_z loss", lz[0, 0].cpu(), r64["cz"][0], r32["cz"][0])
    ck.cmp("generator loss", ld[0, 0].cpu(), r64["dec"][0], r32["dec"][0])
    ck.cmp("hyperbolic distance" if hyper else "mse", ld[0, 1].cpu(), r64["dec"][1], r32["dec"][1])
    _check_step(ck, "cx", sd64, sd32, r64["cx"][1], r32["cx"][1], 1, hyper, after_c)
    _check_step(ck, "cz", sd64, sd32, r64["cz"][1], r32["cz"][1], 1, hyper, after_c)
    for net in ("dec", "enc"):
        _check_step(ck, net, sd64, sd32, r64["dec"][2], r32["dec"][2], 1, hyper, after_g)
    WORST[ck.case] = ck.worst
    print(f"\nsweep {ck.case} [{tag}]: worst errgpu / allowance {ck.worst:.3f}")
    ck.done()


# ------------------------------------------------------------------------------------------------ 2. one iteration of each kind
@pytest.mark.parametrize("case", sc.grid(), ids=sc.grid_id)
def test_one_iteration_of_each_kind_against_fp64(case):
    S, L, B, hyper, tag = case
    _one_of_each(S, L, B, hyper, tag)


def test_train_mode_iterations_at_a_runtime_shape():
    """(65, 20, 48) hyperbolic in train mode: the same injected dropout masks on both sides."""
    S, L, B = 65, 20, 48
    gen = torch.Generator().manual_seed(65)
    dm = lambda: (torch.rand(B, 128, generator=gen) >= 0.2).float() / 0.8
    rm = sc.rand_masks
    masks = dict(cx=dict(valid=rm(gen, B, .25, 4, L), fake=rm(gen, B, .25, 4, L), inter=rm(gen, B, .25, 4, L), dec=dm()),
                 cz=dict(fake=rm(gen, B, .2, 2, L), valid=rm(gen, B, .2, 2, L), inter=rm(gen, B, .2, 2, L)),
                 dec=dict(cz=rm(gen, B, .2, 2, L), cx=rm(gen, B, .25, 4, L), dec_gen=dm(), dec_rec=dm()))
    _one_of_each(S, L, B, True, "train", masks)


# ------------------------------------------------------------------------------------------------ 3. the epoch form (tests/epoch_oracle.py)


def test_epoch_at_a_runtime_shape_with_the_hoisted_critic_phase():
    from hypad_amd.engine import Engine
    assert Engine(65, 20, 48, True).critic_phase_persistent()
    _epoch_against_oracle(65, 20, 48, 1, (0,))


def test_epoch_beyond_the_hoisted_critic_phase_lds_plan():
    """(200, 31, 128): wider than the hoisted phase's LDS plan at latent 31 (the widest window it takes there is 127), so the epoch
    runs its critic phase as per-minibatch launch groups."""
    from hypad_amd import _C
    ws = lambda S: (_C.lib.hypad_epoch_workspace_bytes(ctypes.byref(_C.Dims(S, 31, 128, 1, 1, 0)), NB, NC),
                    _C.lib.hypad_train_workspace_bytes(ctypes.byref(_C.Dims(S, 31, 128, 1, 1, 0))))
    hoisted = [S for S in range(1, 257) if ws(S)[0] != ws(S)[1]]
    assert max(hoisted) == 127 and 200 not in hoisted
    _epoch_against_oracle(200, 31, 128, 1, (0,))


def test_epoch_eight_signal_group_colocated_optimizer():
    """8 models at (113, 20, 64): the co-located dW + Adam build.  Signals 0, 3 and 7 equal the same model run alone, bit for bit."""
    S, L, B, k = 113, 20, 64, 8
    eng, full, (w0, xw, planes, perm) = _epoch_against_oracle(S, L, B, k, (0, 7), seed=3)
    for s in (0, 3, 7):
        one = _engine(S, L, B, True, [w0[s]], seed=7, first_signal=s)
        l = one.train_epoch_graph(cu(xw[s:s + 1]), cu(perm, torch.int32), NB, NC, False,
                                  noise={n: cu(v[:, s:s + 1]) for n, v in planes.items()}).cpu().numpy()
        assert np.array_equal(l[0], full[s]), ("losses", s)
        for net in sc.NETS:
            for which in ("params", "exp_avg", "exp_avg_sq"):
                assert torch.equal(getattr(one, which)[net][0], getattr(eng, which)[net][s]), (s, net, which)


# ------------------------------------------------------------------------------------------------ 4. scoring forward
def _arena(net, sd, S, L, hyper):
    from hypad_amd import _C
    nid = dict(enc=_C.NET_ENCODER, dec=_C.NET_DECODER, cx=_C.NET_CRITIC_X, cz=_C.NET_CRITIC_Z)[net]
    cat, total = _C.param_catalogue(nid, S, L, hyper)
    a = torch.zeros(total, dtype=torch.float32)
    for nm, off, shape in cat:
        n = int(np.prod(shape))
        a[off:off + n] = sd[f"{net}.{nm}"].reshape(-1)
    return a.cuda()


def _score_refs(sd, x, hyper):
    """fp64 / fp32 composition of the test loop's forward: (hyper, eucl, hyper_real, critic, rowdist, latent, critic_z(latent))."""
    out = {}
    for dt in (F64, torch.float32):
        s = sc.cast(sd, dt)
        xx = x.to(dt)
        with torch.no_grad():
            lat, _ = manual.encoder_fwd(xx, s)
            h, e, _ = manual.decoder_fwd(lat, s, hyper)
            r = dict(eucl=e if hyper else h, critic=manual.critic_fwd(xx, manual.critic_layers(s, "cx."))[0][:, 0], lat=lat,
                     cz=manual.critic_fwd(lat, manual.critic_layers(s, "cz."))[0][:, 0])
            if hyper:
                hr, _ = manual.head_fwd(xx, s)
                r.update(hyper=h, hyper_real=hr, rowdist=manual.rowdist_fwd(hr, h))
        out[dt] = r
    return out


SCORE_S, SCORE_L = (8, 64, 65, 113, 129, 256), (7, 20, 32)


@pytest.mark.parametrize("S", SCORE_S)
def test_score_forward_at_runtime_windows(S):
    from hypad_amd import _C
    failures = []
    for L in SCORE_L:
        hyper = True
        sd = sc.init_state(S, L, hyper, seed=S + L)
        arenas = {k: _arena(k, sd, S, L, hyper) for k in sc.NETS}
        nmax = 3001
        g = torch.Generator().manual_seed(S * 100 + L)
        series = (torch.rand(nmax + S - 1, generator=g, dtype=F64) * 2 - 1).float()
        xw = series.unfold(0, S, 1).contiguous()                       # (nmax, S) windows of the series
        refs = _score_refs(sd, xw, hyper)
        ws_bytes = _C.lib.hypad_score_workspace_bytes(S, L, 1)
        ws = torch.empty(max(ws_bytes // 4, 1), device="cuda")
        xw_d, ser_d = xw.cuda(), series.cuda()
        for n in (1, 15, 16, 17, 33, 16 * 7 + 1, nmax):
            for view in ("matrix", "series"):
                ck = sc.Checker(f"score ({S},{L}) rows {n} {view}")
                new = lambda *s: torch.full(s, float("nan"), device="cuda")
                o = dict(hyper=new(n, S), eucl=new(n, S), hyper_real=new(n, S), critic=new(n), rowdist=new(n))
                src, stride = (xw_d, 0) if view == "matrix" else (ser_d, 1)
                _C.check(_C.lib.hypad_score_forward_packed(_C.ptr(arenas["enc"]), _C.ptr(arenas["dec"]), _C.ptr(arenas["cx"]), _C.ptr(src),
                                                           stride, _C.ptr(o["hyper"]), _C.ptr(o["eucl"]), _C.ptr(o["hyper_real"]),
                                                           _C.ptr(o["critic"]), _C.ptr(o["rowdist"]), n, S, L, 1, ws.data_ptr(), ws_bytes,
                                                           _C.stream()), "score_forward_packed")
                for key in o:
                    ck.cmp(key, o[key].cpu(), refs[F64][key][:n], refs[torch.float32][key][:n])
                failures += ck.failures
        # the stand-alone network forwards at the largest row count
        n = nmax
        ck = sc.Checker(f"network forwards ({S},{L}) rows {n}")
        lat, hy, eu, cr, crz = (torch.empty(n, L, device="cuda"), torch.empty(n, S, device="cuda"), torch.empty(n, S, device="cuda"),
                                torch.empty(n, device="cuda"), torch.empty(n, device="cuda"))
        _C.check(_C.lib.hypad_encoder_fwd(_C.ptr(arenas["enc"]), _C.ptr(xw_d), _C.ptr(lat), n, S, L, _C.stream()), "encoder_fwd")
        lat_ref = refs[F64]["lat"].float().cuda()               # the decoder and critic_z are checked on the reference latent
        _C.check(_C.lib.hypad_decoder_fwd(_C.ptr(arenas["dec"]), _C.ptr(lat_ref), _C.ptr(hy), _C.ptr(eu), n, S, L, 1, None, _C.stream()),
                 "decoder_fwd")
        _C.check(_C.lib.hypad_critic_x_fwd(_C.ptr(arenas["cx"]), _C.ptr(xw_d), _C.ptr(cr), n, S, L, None, _C.stream()), "critic_x_fwd")
        _C.check(_C.lib.hypad_critic_z_fwd(_C.ptr(arenas["cz"]), _C.ptr(lat_ref), _C.ptr(crz), n, L, None, _C.stream()), "critic_z_fwd")
        lat32 = refs[F64]["lat"].float()
        r32 = _score_refs_from_latent(sd, lat32, hyper)
        r64 = _score_refs_from_latent(sd, lat32.double(), hyper)
        ck.cmp("encoder", lat.cpu(), refs[F64]["lat"], refs[torch.float32]["lat"])
        ck.cmp("decoder hyper", hy.cpu(), r64["hyper"], r32["hyper"])
        ck.cmp("decoder eucl", eu.cpu(), r64["eucl"], r32["eucl"])
        ck.cmp("critic_x", cr.cpu(), refs[F64]["critic"], refs[torch.float32]["critic"])
        ck.cmp("critic_z", crz.cpu(), r64["cz"], r32["cz"])
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _score_refs_from_latent(sd, lat, hyper):
    s = sc.cast(sd, lat.dtype)
    with torch.no_grad():
        h, e, _ = manual.decoder_fwd(lat, s, hyper)
        return dict(hyper=h, eucl=e, cz=manual.critic_fwd(lat, manual.critic_layers(s, "cz."))[0][:, 0])


@pytest.mark.parametrize("series_view", [False, True])
def test_score_forward_signals_ragged_group_at_a_runtime_window(series_view):
    from hypad_amd import _C
    S, L, counts = 129, 20, (1, 17, 300)
    sds = [sc.init_state(S, L, True, seed=40 + i) for i in range(len(counts))]
    stack = lambda net: torch.stack([_arena(net, sd, S, L, True) for sd in sds]).contiguous()
    enc, dec, cx = stack("enc"), stack("dec"), stack("cx")
    g = torch.Generator().manual_seed(129)
    serieses = [(torch.rand(c + S - 1, generator=g, dtype=F64) * 2 - 1).float() for c in counts]
    wins = [s.unfold(0, S, 1).contiguous() for s in serieses]
    parts = serieses if series_view else wins
    row_off = np.cumsum([0] + list(counts)).tolist()
    x_off = np.cumsum([0] + [p.numel() for p in parts])[:-1].tolist()
    x = torch.cat([p.reshape(-1) for p in parts]).cuda()
    n = row_off[-1]
    o = dict(hyper=torch.full((n, S), float("nan"), device="cuda"), eucl=torch.full((n, S), float("nan"), device="cuda"),
             hyper_real=torch.full((n, S), float("nan"), device="cuda"), critic=torch.full((n,), float("nan"), device="cuda"),
             rowdist=torch.full((n,), float("nan"), device="cuda"))
    ws_bytes = _C.lib.hypad_score_signals_workspace_bytes(S, L, 1, len(counts))
    ws = torch.empty(max(ws_bytes // 4, 1), device="cuda")
    _C.check(_C.lib.hypad_score_forward_signals(_C.ptr(enc), _C.ptr(dec), _C.ptr(cx), len(counts), _C.int64s(row_off), _C.int64s(x_off),
                                                _C.ptr(x), 1 if series_view else S, _C.ptr(o["hyper"]), _C.ptr(o["eucl"]),
                                                _C.ptr(o["hyper_real"]), _C.ptr(o["critic"]), _C.ptr(o["rowdist"]), S, L, 1, ws.data_ptr(),
                                                ws_bytes, _C.stream()), "score_forward_signals")
    failures = []
    for i, sd in enumerate(sds):
        refs = _score_refs(sd, wins[i], True)
        ck = sc.Checker(f"score signals ({S},{L}) signal {i} of {counts}")
        for key in o:
            ck.cmp(key, o[key][row_off[i]:row_off[i + 1]].cpu(), refs[F64][key], refs[torch.float32][key])
        failures += ck.failures
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 5. stand-alone Poincare-ball kernels
DIMS = (1, 3, 63, 64, 65, 127, 128, 129, 255, 256)
ROWS = (1, 2, 3, 5, 4 * 9 + 3)


def _op_check(ck, name, gpu_fn, ref_fn, ins, gout, unaligned=False):
    """forward and backward of gpu_fn against ref_fn on fp64 and fp32 autograd"""
    din = [(_unaligned(t.cuda()) if unaligned else t.cuda()).requires_grad_(True) for t in ins]
    out = gpu_fn(*din)
    grads = torch.autograd.grad(out, din, gout.cuda())
    res = {}
    for dt in (F64, torch.float32):
        r = [t.to(dt).requires_grad_(True) for t in ins]
        o = ref_fn(*r)
        res[dt] = (o.detach(), torch.autograd.grad(o, r, gout.to(dt)))
    ck.cmp(name, out.detach().cpu(), res[F64][0], res[torch.float32][0])
    for i, gg in enumerate(grads):
        ck.cmp(f"{name} grad{i}", gg.cpu(), res[F64][1][i], res[torch.float32][1][i])


# Data scale: the 1 - 1e-3 row goes where it is the point (project's limit, logmap0, mobius_add's x).  A distance with an operand
# there, or mobius_add with both operands near the rim, has condition ~1 / (1 - |u|^2) = 500 in fp32: the fp32 oracle's own error is
# then a matter of luck in one reduction order, and the rule measures nothing.  Those operands stay within radius 0.95 / 0.5.
def _gmath_ops():
    from hypad_amd.hyperspace import gmath
    return [
        ("expmap0", lambda u: gmath.expmap0(u, k=-1.0), og.expmap0, (dict(tangent=True),)),
        # (logmap0 of a zero row: artanh(1e-15) / 1e-15 has no fp32 meaning -- its gradient is rounding noise on both sides)
        ("logmap0", lambda y: gmath.logmap0(y, k=-1.0), og.logmap0, (dict(zero_row=False),)),
        ("project", lambda x: gmath.project(x, k=-1.0), lambda x: og.project(x, eps=4e-3), (dict(),)),
        ("mobius_add", lambda x, y: gmath.mobius_add(x, y, k=-1.0), og.mobius_add, (dict(), dict(edge=False, radius=0.5))),
        ("poincare_rowdist", gmath.poincare_rowdist, og.rowwise_poincare_distance, (dict(edge=False), dict(edge=False))),
    ]


@pytest.mark.parametrize("dim", DIMS)
def test_ball_row_kernels_every_layout(dim):
    from hypad_amd.hyperspace import gmath
    failures = []
    g = torch.Generator().manual_seed(dim)
    for rows in ROWS:
        for name, fn, ref, kinds in _gmath_ops():
            ins = [_ball_rows(g, rows, dim, **kind) for kind in kinds]
            oshape = (rows,) if name == "poincare_rowdist" else (rows, dim)
            gout = torch.randn(*oshape, generator=g)
            for unaligned in ((False, True) if rows == 39 else (False,)):
                ck = sc.Checker(f"{name} dim {dim} rows {rows}{' unaligned' if unaligned else ''}")
                _op_check(ck, name, fn, ref, ins, gout, unaligned)
                failures += ck.failures
        # one-row (broadcast) y of mobius_add, and the hyperbolic loss
        ck = sc.Checker(f"dim {dim} rows {rows}")
        x, y = _ball_rows(g, rows, dim), _ball_rows(g, 1, dim, radius=0.5)[0]
        gout = torch.randn(rows, dim, generator=g)
        _op_check(ck, "mobius_add broadcast y", lambda a, b: gmath.mobius_add(a, b, k=-1.0), lambda a, b: og.mobius_add(a, b.unsqueeze(0)),
                  [x, y], gout)
        u, v = _ball_rows(g, rows, dim, edge=False), _ball_rows(g, rows, dim, edge=False)
        _op_check(ck, "hyperbolic_loss", lambda a, b: gmath.hyperbolic_loss(a, b, 7), lambda a, b: og.rowwise_poincare_distance(a, b).sum() / 7,
                  [u, v], torch.tensor(1.3))
        failures += ck.failures
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("dim", (3, 65, 129))
def test_ball_row_kernels_beyond_one_grid_stride(dim):
    """70 001 rows: more than the 65 536 one grid of the row kernels covers (the rest grid-strides)."""
    failures = []
    g = torch.Generator().manual_seed(70001 + dim)
    for name, fn, ref, kinds in _gmath_ops():
        ins = [_ball_rows(g, 70001, dim, **kind) for kind in kinds]
        gout = torch.randn(*((70001,) if name == "poincare_rowdist" else (70001, dim)), generator=g)
        ck = sc.Checker(f"{name} dim {dim} rows 70001")
        _op_check(ck, name, fn, ref, ins, gout)
        failures += ck.failures
    assert not failures, "\n".join(failures)


def test_training_refuses_shapes_its_critic_launches_cannot_hold():
    """(256, 32, 32) -- inside hypad_limits -- needs 164 544 bytes of LDS for the stand-alone critic_x pass: the training calls refuse it
    with HYPAD_EUNSUPPORTED before any launch (they used to fail in hipFuncSetAttribute and leave the HIP error behind for the next
    call).  The grid runs (256, 28, 32) in its place: the same window and row-layout class."""
    from hypad_amd import _C
    from hypad_amd.engine import Engine
    with pytest.raises(_C.HypadError):
        Engine(256, 32, 32, True)
    d = _C.Dims(256, 32, 32, 1, 1, 0)
    st = _C.TrainState(_C.Nets(), _C.Nets(), _C.Nets(), None, 5e-4, 0.9, 0.999, 1e-8, 1e-5, 10)     # (no buffers: nothing may launch)
    io = _C.IterIO()
    for fn in (_C.lib.hypad_critic_x_iteration, _C.lib.hypad_critic_z_iteration, _C.lib.hypad_decoder_iteration):
        assert fn(ctypes.byref(d), ctypes.byref(st), ctypes.byref(io), _C.stream()) == HYPAD_EUNSUPPORTED
    torch.cuda.synchronize()
    torch.zeros(4, device="cuda").add_(1)                  # no HIP error left behind
    Engine(256, 28, 32, True)
    Engine(240, 32, 32, True)


def test_row_kernels_refuse_dim_257():
    from hypad_amd import _C
    a, out = torch.zeros(4, 257, device="cuda"), torch.full((4, 257), 7.0, device="cuda")
    for fn in ("hypad_expmap0_fwd", "hypad_logmap0_fwd", "hypad_project_fwd"):
        assert getattr(_C.lib, fn)(_C.ptr(a), _C.ptr(out), 4, 257, _C.stream()) == HYPAD_EUNSUPPORTED, fn
    assert _C.lib.hypad_mobius_add_fwd(_C.ptr(a), _C.ptr(a), _C.ptr(out), 4, 257, 1, _C.stream()) == HYPAD_EUNSUPPORTED
    d = torch.empty(4, device="cuda")
    assert _C.lib.hypad_poincare_rowdist_fwd(_C.ptr(a), _C.ptr(a), _C.ptr(d), 4, 257, _C.stream()) == HYPAD_EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())                      # nothing ran


@pytest.mark.parametrize("dim", (5, 64, 129, 256))
def test_pairwise_distance_tiles(dim):
    from hypad_amd.hyperspace.poincare_distance import poincare_distance
    failures = []
    g = torch.Generator().manual_seed(dim)
    for n in (1, 63, 64, 65, 130):
        for m in (1, 63, 64, 65, 130):
            a, b = _ball_rows(g, n, dim, edge=False), _ball_rows(g, m, dim, edge=False)
            ck = sc.Checker(f"pairdist dim {dim} {n} x {m}")
            got = poincare_distance(a.cuda(), b.cuda()).cpu()
            ck.cmp("pairdist", got, og.pairwise_poincare_distance(a.double(), b.double()), og.pairwise_poincare_distance(a, b))
            failures += ck.failures
    assert not failures, "\n".join(failures)
