"""The row-wise Riemannian optimiser steps (csrc/riemann_opt.hip: hypad_radam_rows_step, hypad_rsgd_rows_step; hypad_amd.optim's
RiemannianAdam(manifold_rows=True) and RiemannianSGD) against their restatement tests/riemann_opt_ref.py in fp64.

What is compared, all under ``sweep_common.Ck`` unchanged (errgpu <= C * err32 + F, err32 from the same restatement run in fp32 on the
CPU; ``steps=T`` for a recurrence of T steps): the state tensors and, as in tests/test_gpu_optimizer_steps.py and for its reason, the
parameter as the STEP (p_new - p_old) / lr -- comparing p_new itself lets a wrong step hide under max(1, |p|).  The entry points take
their hyper-parameters as C floats, so both sides get the same floats (``f32``).

Data of the one-step sweep.  Ball rows from the origin to radius 0.95 with a zero row (``_ball_rows``), unit rows for the sphere, plain
rows for the untagged case; gradients ~ N(0, 1).  Where the rows allow: row 1 is the RIM row -- a ball row at radius 0.99595, 5e-5 inside
project's limit 1 - 4e-3, with fresh moments and a gradient of norm 1000 along -x, so that the step points outward (SGD's step there is lr |g| / lambda^2 = 8e-4, Adam's
from fresh moments at least 0.48 lr / lambda = 1e-4 -- at step 10 --, either ends beyond the limit: project clamps, asserted on the fp64 reference), and on the sphere a row
whose gradient is parallel to x; row 2 has a zero gradient.  Moments as in the optimizer test: m ~ 0.1 N(0, 1), v = mean(m^2) + U(0, 0.01)
as ONE value per row, every fifth row fresh zeros.  stabilize = 10: steps 10 and 1000 stabilise, 1 and 2 do not.
"""
import os
import re

import numpy as np
import pytest
import torch

import riemann_opt_ref as ref
from oracle import manual
from sweep_common import C as RULE_C
from sweep_common import SENTINEL, Ck, _at_offset, _ball_rows, _guarded, _guards_intact

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
HYPAD_OK, HYPAD_EINVAL, HYPAD_EUNSUPPORTED = 0, -1, -3      # include/hypad.h
f32 = lambda x: float(np.float32(x))
LR, B1, B2, EPS = f32(0.05), f32(0.9), f32(0.999), f32(1e-8)
STEPS, WDS, STAB = (1, 2, 10, 1000), (0.0, f32(0.1)), 10
DIMS, ROWS = (1, 2, 63, 64, 65, 255, 256), (1, 3, 4, 5)
# (momentum, dampening, nesterov)
SGD_CFGS = ((0.0, 0.0, False), (f32(0.9), 0.0, False), (f32(0.9), f32(0.1), False), (f32(0.9), 0.0, True))
ADAM_CFGS = (None,)
KERNELS = [("adam", "ball"), ("adam", "sphere"), ("sgd", "ball"), ("sgd", "sphere"), ("sgd", "euclidean")]
MAN_ID = {"euclidean": 0, "ball": 1, "sphere": 2}            # HYPAD_MANIFOLD_*
RIM_RADIUS = 0.99595


def _grid_rows():
    """Rows one pass of the kernels' grid covers, from the source: wave_grid's cap on the blocks times the waves of a block."""
    src = open(os.path.join(ROOT, "hypad_amd", "csrc", "riemann_opt.hip")).read()
    threads = int(re.search(r"constexpr int THREADS = (\d+);", src).group(1))
    assert "constexpr int WAVES = THREADS / 64;" in src
    cap = re.search(r"b > (\d+) \? (\d+) :", src[src.index("inline int wave_grid"):])
    assert cap and cap.group(1) == cap.group(2)
    return int(cap.group(1)) * (threads // 64)


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks, what):
    print(f"\nriemannian rows {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f} over {len(cks)} cases")
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ data
def _data(g, rule, man, rows, dim):
    """(x, grad, states, rim): states (m, v) for Adam, (buf,) for SGD (dropped by the caller where momentum == 0); rim: the rim row or None."""
    rim = None
    grad = torch.randn(rows, dim, generator=g)
    if man == "ball":
        x = _ball_rows(g, rows, dim, edge=False, radius=0.95)
        if rows >= 3:
            rim = 1
            u = torch.randn(dim, generator=g, dtype=F64)
            u = u / u.norm()
            x[1], grad[1] = (u * RIM_RADIUS).float(), (u * -1000).float()      # (the step is along -grad: outward)
    elif man == "sphere":
        a = torch.randn(rows, dim, generator=g, dtype=F64)
        x = (a / a.norm(dim=1, keepdim=True)).float()
        if rows >= 3:
            grad[1] = -2.5 * x[1]                                  # parallel to x: no tangent component
    else:
        x = torch.rand(rows, dim, generator=g) * 0.2 - 0.1
    if rows >= 4:
        grad[2] = 0.0
    m = 0.1 * torch.randn(rows, dim, generator=g)
    v = ((m * m).mean(1, keepdim=True) + 0.01 * torch.rand(rows, 1, generator=g)).expand(rows, dim).contiguous()
    fresh = torch.arange(rows) % 5 == 0
    if rim is not None:
        fresh[rim] = True
    m[fresh], v[fresh] = 0.0, 0.0
    return x, grad, ((m, v) if rule == "adam" else (m,)), rim


def _states(rule, cfg, st):
    return st if rule == "adam" or cfg[0] != 0 else ()


# ------------------------------------------------------------------------------------------------ the two sides
def _gpu(rule, man, x, grad, st, step, lr, wd, cfg, dev=lambda t: t.cuda(), sync=True):
    """One step through the C ABI -> (x, *states) on the host, and the device gradient."""
    c = _C()
    X, G = dev(x), dev(grad)
    S = [dev(s) for s in st]
    rows, dim = x.shape
    if rule == "adam":
        rc = c.lib.hypad_radam_rows_step(c.ptr(X), c.ptr(G), c.ptr(S[0]), c.ptr(S[1]), rows, dim, MAN_ID[man], step, lr, B1, B2, EPS, wd, STAB, c.stream())
    else:
        mu, damp, nest = cfg
        rc = c.lib.hypad_rsgd_rows_step(c.ptr(X), c.ptr(G), c.ptr(S[0]) if S else None, rows, dim, MAN_ID[man], step, lr, mu, damp, wd, int(nest), STAB,
                                        c.stream())
    c.check(rc, f"{rule} {man}")
    if sync:
        torch.cuda.synchronize()
    return (X, *S), G


def _ref(rule, man, x, grad, st, step, lr, wd, cfg, dt):
    X, G = x.to(dt), grad.to(dt)
    S = [s.to(dt) for s in st]
    M = ref.MANIFOLDS[man]
    if rule == "adam":
        return ref.radam_rows(M, X, G, S[0], S[1], step, lr, B1, B2, EPS, wd, STAB)
    mu, damp, nest = cfg
    y, b = ref.rsgd_rows(M, X, G, S[0] if S else None, step, lr, mu, damp, wd, nest, STAB)
    return (y,) if b is None else (y, b)


NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}


def _compare(ck, rule, x, lr, got, r64, r32, steps=1):
    for name, a, b, c in zip(NAMES[rule], got[1:], r64[1:], r32[1:]):
        ck.cmp(name, a, b, c, steps=steps)
    po = x.double()
    ck.cmp("step (p_new - p_old) / lr", (got[0].double().cpu() - po) / lr, (r64[0] - po) / lr, (r32[0].double() - po) / lr, steps=steps)


def _uniform_rows(ck, v):
    bad = torch.nonzero((v != v[:, :1]).any(1))
    if len(bad):
        r = int(bad[0])
        ck.failures.append(f"{ck.case}: row {r} of exp_avg_sq is not one value repeated: {v[r].unique().tolist()[:4]}")


def _case(rule, man, g, rows, dim, step, wd, cfg, cks):
    x, grad, st, rim = _data(g, rule, man, rows, dim)
    st = _states(rule, cfg, st)
    ck = Ck(f"{rule} {man} rows {rows} D {dim} step {step} wd {wd:g} cfg {cfg}")
    got, G = _gpu(rule, man, x, grad, st, step, LR, wd, cfg)
    got = [t.cpu() for t in got]
    r64, r32 = (_ref(rule, man, x, grad, st, step, LR, wd, cfg, dt) for dt in (F64, F32))
    if rim is not None:
        assert abs(float(r64[0][rim].norm()) - manual.MAXNORM_F32) < 1e-12, f"{ck.case}: the reference's rim row does not end on project's limit"
    _compare(ck, rule, x, LR, got, r64, r32)
    if rule == "adam":
        _uniform_rows(ck, got[2])
    if not torch.equal(G.cpu(), grad):
        ck.failures.append(f"{ck.case}: the gradient was written to")
    cks.append(ck)


def _cfgs(rule):
    return ADAM_CFGS if rule == "adam" else SGD_CFGS


# ================================================================================================ 1. one step, every launch edge
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rule,man", KERNELS)
def test_one_step(rule, man, dim):
    """D at the lane and element-per-lane edges, rows around one block's four waves, steps 1 / 2 / 10 / 1000 from given moments, weight
    decay 0 and 0.1, SGD without momentum, with it, with dampening and with Nesterov's form."""
    g = torch.Generator().manual_seed(100 * dim + 7 * len(rule) + len(man))
    cks = []
    for rows in ROWS:
        for step in STEPS:
            for wd in WDS:
                for cfg in _cfgs(rule):
                    _case(rule, man, g, rows, dim, step, wd, cfg, cks)
    _finish(cks, f"{rule} {man} D {dim}")


@pytest.mark.parametrize("rule,man", KERNELS)
def test_one_step_past_the_grid(rule, man):
    """D = 20 and one pass of the capped grid plus a partial block of rows: the grid stride."""
    rows = _grid_rows() + 5
    assert rows == 4 * 4096 + 5
    g = torch.Generator().manual_seed(len(rule) + 3 * len(man))
    cks = []
    for cfg in _cfgs(rule)[-2:]:
        _case(rule, man, g, rows, 20, 10, WDS[1], cfg, cks)
    _finish(cks, f"{rule} {man} rows {rows}")


# ================================================================================================ 2. rows do not see each other
@pytest.mark.parametrize("rule,man", KERNELS)
def test_a_row_gets_the_bits_it_gets_alone(rule, man):
    g = torch.Generator().manual_seed(11)
    for dim in (20, 256):
        x, grad, st, _ = _data(g, rule, man, 6, dim)
        for cfg in _cfgs(rule)[-2:]:
            s = _states(rule, cfg, st)
            whole = [t.cpu() for t in _gpu(rule, man, x, grad, s, 10, LR, WDS[1], cfg)[0]]
            for r in range(6):
                alone = [t.cpu() for t in _gpu(rule, man, x[r:r + 1], grad[r:r + 1], [t[r:r + 1] for t in s], 10, LR, WDS[1], cfg)[0]]
                for name, a, b in zip(("p",) + NAMES[rule], whole, alone):
                    assert torch.equal(a[r:r + 1], b), f"{rule} {man} D {dim} cfg {cfg}: {name} of row {r} depends on the rows around it"
            if rule == "adam":
                assert bool((whole[2] == whole[2][:, :1]).all())


# ================================================================================================ 3. memory discipline
@pytest.mark.parametrize("rule,man", KERNELS)
def test_operands_at_storage_offset_one_between_guards(rule, man):
    """Every operand at storage offset 1; every written buffer between two sentinel words that stay; the gradient unchanged; the bits of
    the aligned call."""
    g = torch.Generator().manual_seed(13)
    for rows, dim in ((5, 63), (3, 256)):
        x, grad, st, _ = _data(g, rule, man, rows, dim)
        cfg = _cfgs(rule)[-1]
        st = _states(rule, cfg, st)
        want = [t.cpu() for t in _gpu(rule, man, x, grad, st, 10, LR, WDS[1], cfg)[0]]
        offs = []

        def dev(t):
            if t is grad:
                return _at_offset(t.cuda(), 1)
            buf, v = _guarded(t.shape, 1)                          # (the sentinel in front is the buffer's word 0)
            v.copy_(t)
            offs.append((buf, 1))
            return v
        got, G = _gpu(rule, man, x, grad, st, 10, LR, WDS[1], cfg, dev=dev)
        assert len(offs) == 1 + len(st)
        for buf, off in offs:
            assert _guards_intact(buf, off), f"{rule} {man} ({rows}, {dim}): a guard word around a written buffer changed"
        assert torch.equal(G.cpu(), grad)
        for name, a, b in zip(("p",) + NAMES[rule], got, want):
            assert torch.equal(a.cpu(), b), f"{rule} {man} ({rows}, {dim}): {name} at storage offset 1 differs from the aligned call"


# ================================================================================================ 4. argument checks
def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    c = _C()
    rows, dim = 3, 100
    bufs = [torch.full((rows * 257,), SENTINEL, device="cuda") for _ in range(4)]
    P, G, M, V = (c.ptr(t) for t in bufs)
    s = c.stream()
    ahp, shp = (LR, B1, B2, EPS, WDS[1], STAB), (LR, f32(0.9), 0.0, WDS[1], 0, STAB)
    radam = lambda p=P, g=G, m=M, v=V, rows=rows, dim=dim, man=1, step=1: c.lib.hypad_radam_rows_step(p, g, m, v, rows, dim, man, step, *ahp, s)
    rsgd = lambda p=P, g=G, b=M, rows=rows, dim=dim, man=1, step=1, hp=shp: c.lib.hypad_rsgd_rows_step(p, g, b, rows, dim, man, step, *hp, s)
    for call in (radam, rsgd):
        assert call(rows=-1) == HYPAD_EINVAL and call(dim=0) == HYPAD_EINVAL and call(dim=-4) == HYPAD_EINVAL
        assert call(step=0) == HYPAD_EINVAL and call(man=3) == HYPAD_EINVAL and call(man=-1) == HYPAD_EINVAL
        assert call(p=None) == HYPAD_EINVAL and call(g=None) == HYPAD_EINVAL
        assert call(dim=257) == HYPAD_EUNSUPPORTED
        assert call(rows=2 ** 31 // 100 + 1) == HYPAD_EUNSUPPORTED                     # rows * dim beyond int
        assert call(rows=-1, dim=257) == HYPAD_EINVAL and call(dim=257, p=None) == HYPAD_EUNSUPPORTED      # sizes, then limits, then operands
        assert call(rows=0) == HYPAD_OK and call(rows=0, p=None, g=None) == HYPAD_OK
    assert radam(man=0) == HYPAD_EINVAL                                                # Adam has no plain-row form here
    assert radam(m=None) == HYPAD_EINVAL and radam(v=None) == HYPAD_EINVAL
    assert rsgd(b=None) == HYPAD_EINVAL                                                # momentum without a buffer
    assert rsgd(hp=(LR, 0.0, 0.0, WDS[1], 0, STAB)) == HYPAD_EINVAL                    # a buffer without momentum
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in bufs)                              # nothing ran
    assert rsgd(man=0) == HYPAD_OK and rsgd(b=None, hp=(LR, 0.0, 0.0, WDS[1], 0, STAB)) == HYPAD_OK    # ... and these do run
    torch.cuda.synchronize()
    assert not bool((bufs[0][:rows * dim] == SENTINEL).any()) and bool((bufs[0][rows * dim:] == SENTINEL).all())


# ================================================================================================ 5. the optimiser classes
def _param(x, man):
    from hypad_amd.hyperspace import hyrnn_nets as hn
    if man == "euclidean":
        return torch.nn.Parameter(x.cuda())
    return hn.ManifoldParameter(x.cuda(), manifold=hn.PoincareBall() if man == "ball" else hn.Sphere())


def test_a_ball_vector_keeps_its_step_under_manifold_rows():
    from hypad_amd import optim
    g = torch.Generator().manual_seed(17)
    x = _ball_rows(g, 1, 100, radius=0.9)[0]
    grads = [torch.randn(100, generator=g) for _ in range(12)]
    runs = []
    for flag in (False, True):
        p = _param(x, "ball")
        opt = optim.RiemannianAdam([p], lr=LR, weight_decay=1e-5, stabilize=10, manifold_rows=flag)
        for gr in grads:
            p.grad = gr.cuda()
            opt.step()
        runs.append((p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("man", ("ball", "sphere"))
@pytest.mark.parametrize("rule", ("adam", "sgd", "sgd-dampened", "sgd-nesterov"))
def test_twenty_steps_of_the_optimiser_classes(rule, man):
    """(6, 20), 20 steps driven by a recorded sequence of gradients (self-computed ones would let Adam's sign-like first steps diverge
    chaotically), fresh state, weight decay 0.1, stabilize 10; the classes drive the GPU side: state creation, the host-side clone of
    the first gradient into the momentum buffer, the step counter.  Compared after every step under the rule with steps = 20."""
    from hypad_amd import optim
    T = 20
    g = torch.Generator().manual_seed(19)
    x, _, _, _ = _data(g, "adam", man, 6, 20)
    if man == "ball":
        x[1] = x[0] * 0.5                                          # (no rim row here: a parameter a training run would hold)
    grads = [torch.randn(6, 20, generator=g) for _ in range(T)]
    M = ref.MANIFOLDS[man]
    p = _param(x, man)
    if rule == "adam":
        opt = optim.RiemannianAdam([p], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WDS[1], stabilize=STAB, manifold_rows=True)
        r64, r32 = (ref.radam_run(M, x.to(dt), grads, LR, B1, B2, EPS, WDS[1], STAB) for dt in (F64, F32))
        keys = ("exp_avg", "exp_avg_sq")
    else:
        mu, damp, nest = SGD_CFGS[{"sgd": 1, "sgd-dampened": 2, "sgd-nesterov": 3}[rule]]
        opt = optim.RiemannianSGD([p], lr=LR, momentum=mu, dampening=damp, weight_decay=WDS[1], nesterov=nest, stabilize=STAB)
        r64, r32 = (ref.rsgd_run(M, x.to(dt), grads, LR, mu, damp, WDS[1], nest, STAB) for dt in (F64, F32))
        keys = ("momentum_buffer",)
    ck = Ck(f"{rule} {man} (6, 20) over {T} steps")
    for t, gr in enumerate(grads, 1):
        p.grad = gr.cuda()
        opt.step()
        st = opt.state[p]
        assert st["step"] == t and opt.param_groups[0]["step"] == t
        ck.cmp(f"p after step {t}", p.detach(), r64[t - 1][0], r32[t - 1][0], steps=T)
        for k, key in enumerate(keys, 1):
            ck.cmp(f"{key} after step {t}", st[key], r64[t - 1][k], r32[t - 1][k], steps=T)
        assert torch.equal(p.grad.cpu(), gr)
    # ... and the whole displacement as a step: (p_T - p_0) / (T lr)
    po = x.double()
    ck.cmp("(p_T - p_0) / (T lr)", (p.detach().double().cpu() - po) / (T * LR), (r64[-1][0] - po) / (T * LR), (r32[-1][0].double() - po) / (T * LR), steps=T)
    assert set(opt.state[p]) == {"step", *keys}
    _finish([ck], f"{rule} {man} trajectory")


def test_untagged_parameters_under_riemannian_sgd():
    """An untagged parameter whose last dimension no row holds, (3, 300): the plain rule on rows of its own making, against the
    restatement; without momentum it keeps no buffer."""
    from hypad_amd import optim
    g = torch.Generator().manual_seed(23)
    x = torch.randn(3, 300, generator=g) * 0.1
    grads = [torch.randn(3, 300, generator=g) for _ in range(3)]
    for mu in (0.0, f32(0.9)):
        p = _param(x, "euclidean")
        opt = optim.RiemannianSGD([p], lr=LR, momentum=mu, weight_decay=WDS[1])
        r64, r32 = (ref.rsgd_run(ref.EuclideanRows, x.to(dt), grads, LR, mu, 0.0, WDS[1]) for dt in (F64, F32))
        for gr in grads:
            p.grad = gr.cuda()
            opt.step()
        ck = Ck(f"RiemannianSGD untagged (3, 300) momentum {mu:g}")
        po = x.double()
        ck.cmp("(p_3 - p_0) / (3 lr)", (p.detach().double().cpu() - po) / (3 * LR), (r64[-1][0] - po) / (3 * LR), (r32[-1][0].double() - po) / (3 * LR), steps=3)
        if mu:
            ck.cmp("momentum_buffer", opt.state[p]["momentum_buffer"], r64[-1][1], r32[-1][1], steps=3)
        else:
            assert "momentum_buffer" not in opt.state[p]
        ck.done()


@pytest.mark.parametrize("rule,man", KERNELS)
def test_a_step_on_a_side_stream_gives_the_default_stream_its_bits(rule, man):
    g = torch.Generator().manual_seed(29)
    x, grad, st, _ = _data(g, rule, man, 5, 65)
    cfg = _cfgs(rule)[-1]
    st = _states(rule, cfg, st)
    want = [t.cpu() for t in _gpu(rule, man, x, grad, st, 10, LR, WDS[1], cfg)[0]]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, _ = _gpu(rule, man, x, grad, st, 10, LR, WDS[1], cfg, sync=False)       # (the copies to the device are issued on `side` too)
    side.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a.cpu(), b)


# ================================================================================================ 6. it trains
@pytest.mark.parametrize("which", ("adam", "sgd"))
def test_the_hyperplane_layer_trains_on_its_manifolds(which):
    """MobiusDist2Hyperplane(20, 6) fitted to 32 fixed ball rows with cross-entropy for 30 steps over scale, point and tangent.  The loss
    falls; every point stays inside the ball; every tangent row keeps norm 1 -- to C times what the fp32 restatement of the sphere's rule
    loses on the same run (the recorded gradients of tangent), C the comparison rule's.  No parity claim."""
    from hypad_amd import optim
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(31)
    g = torch.Generator().manual_seed(31)
    layer = hyrnn_nets.MobiusDist2Hyperplane(20, 6).cuda()
    x = _ball_rows(g, 32, 20, edge=False, zero_row=False, radius=0.9).cuda()
    target = torch.randint(0, 6, (32,), generator=g).cuda()
    params = [layer.scale, layer.point, layer.tangent]
    lr = f32(0.05)
    if which == "adam":
        opt = optim.RiemannianAdam(params, lr=lr, stabilize=STAB, manifold_rows=True)
    else:
        opt = optim.RiemannianSGD(params, lr=lr, momentum=f32(0.9), stabilize=STAB)
    t0 = layer.tangent.detach().cpu().clone()
    losses, tgrads = [], []
    for _ in range(30):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(layer(x), target)
        loss.backward()
        tgrads.append(layer.tangent.grad.detach().cpu().clone())
        opt.step()
        losses.append(float(loss.detach()))
    losses.append(float(torch.nn.functional.cross_entropy(layer(x), target).detach()))
    print(f"\n{which}: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] < losses[0] and all(np.isfinite(losses))
    point, tangent = layer.point.detach().cpu(), layer.tangent.detach().cpu()
    assert bool(torch.isfinite(point).all()) and float(point.double().norm(dim=1).max()) < 1.0
    if which == "adam":
        run32 = ref.radam_run(ref.SphereRows, t0, tgrads, lr, 0.9, 0.999, 1e-8, 0.0, STAB)
    else:
        run32 = ref.rsgd_run(ref.SphereRows, t0, tgrads, lr, f32(0.9), 0.0, 0.0, False, STAB)
    dev32 = max(float((s[0].double().norm(dim=1) - 1).abs().max()) for s in run32)
    dev = float((tangent.double().norm(dim=1) - 1).abs().max())
    print(f"{which}: | |tangent row| - 1 | {dev:.3e}, the fp32 restatement's on the same gradients {dev32:.3e}")
    assert bool(torch.isfinite(tangent).all()) and dev <= RULE_C * dev32
