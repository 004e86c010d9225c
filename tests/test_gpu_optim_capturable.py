"""The grouped, capturable optimiser steps (csrc/optim_group.hip: hypad_optim_step_advance, hypad_optim_group_adam, hypad_optim_group_sgd;
hypad_amd.optim's ``capturable=True``) against their restatement in fp64 -- tests/riemann_opt_ref.py for ball and sphere rows and SGD's
plain rows, tests/optim_group_ref.py for the element-wise Adam of a plain tensor -- and, captured into a graph with forward and backward,
against the same steps run eagerly.

The yardstick is ``sweep_common.Ck`` unchanged (errgpu <= 8 * err32 + 2e-6, err32 from the same restatement run in fp32 on the CPU;
``steps=T`` for T steps), used as tests/test_gpu_riemann_opt.py uses it: the state tensors as they are and the parameter as the STEP
(p_new - p_old) / lr.  The data of a ball or sphere tensor is that file's ``_data`` with its special rows -- (3, D): row 1 the rim row
on which project clamps (ball) or the gradient along x (sphere), the last ball row zero -- and row 0's gradient set to zero here.
Where two GPU runs are compared (a captured step with an eager one, a position in the list with another, the step number by value
with the device counter), they are compared bit for bit.  Two comparisons have no restatement on the CPU, because the model's forward
and backward run only on the GPU: the capturable against the default optimiser over nine training steps, and the state round trip
into a default optimiser.  There the default optimiser's result stands for both references, so err32 = 0 and the whole allowance is
the rule's floor, steps * 2e-6.
"""
import copy
import os
import re

import numpy as np
import pytest
import torch

import optim_group_ref as gref
from oracle import manual
from sweep_common import SENTINEL, Ck, _at_offset, _ball_rows, _guarded, _guards_intact
from test_gpu_riemann_opt import _data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
HYPAD_OK, HYPAD_EINVAL, HYPAD_EUNSUPPORTED = 0, -1, -3      # include/hypad.h
f32 = lambda x: float(np.float32(x))
LR, B1, B2, EPS = f32(0.05), f32(0.9), f32(0.999), f32(1e-8)
STEPS, WDS, STAB = (1, 2, 10, 1000), (0.0, f32(0.1)), 10
DIMS = (1, 2, 63, 64, 65, 255, 256)
PLAIN = (1, 255, 256, 257, 513)
# Adam: (b1, b2, eps); SGD: (momentum, dampening, nesterov)
CFGS = {"adam": ((B1, B2, EPS),), "sgd": ((0.0, 0.0, False), (f32(0.9), 0.0, False), (f32(0.9), f32(0.1), False), (f32(0.9), 0.0, True))}
MAN_ID = {"euclidean": 0, "ball": 1, "sphere": 2}            # HYPAD_MANIFOLD_*
NAMES = {"adam": ("exp_avg", "exp_avg_sq"), "sgd": ("momentum_buffer",)}
GROUP_MAX = 32


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks, what):
    print(f"\ngrouped step {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f} over {len(cks)} cases")
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ data
def _tensor(g, rule, man, rows, dim, numel=None):
    """(man, x, grad, [states]) on the host: a manifold's tensor (rows, dim), a plain one (numel,)."""
    if man != "euclidean":
        x, grad, st, _ = _data(g, rule, man, rows, dim)
        if rows >= 3:
            grad[0] = 0.0
        return man, x, grad, list(st)
    x = torch.rand(numel, generator=g) * 0.2 - 0.1
    grad = torch.randn(numel, generator=g)
    m = 0.1 * torch.randn(numel, generator=g)
    v = m * m * torch.rand(numel, generator=g) + 0.01 * torch.rand(numel, generator=g)
    if numel % 2 == 0:                                             # fresh moments
        m, v = torch.zeros(numel), torch.zeros(numel)
    return man, x, grad, ([m, v] if rule == "adam" else [m])


def _mixed(g, rule, dim):
    """All kinds in one list: ball (3, D), sphere (3, D), plain tensors of 1, 255, 256, 257 and 513 elements, a rank-1 ball vector."""
    out = [_tensor(g, rule, "ball", 3, dim), _tensor(g, rule, "sphere", 3, dim)]
    out += [_tensor(g, rule, "euclidean", 0, 0, n) for n in PLAIN]
    return out + [_tensor(g, rule, "ball", 1, dim)]


def _with_cfg(rule, cfg, tensors):
    """SGD without momentum keeps no buffer."""
    return [(man, x, gr, st if rule == "adam" or cfg[0] != 0 else []) for man, x, gr, st in tensors]


EMPTY = ("empty", None, None, [])


# ------------------------------------------------------------------------------------------------ the GPU side
def _plan(man, x):
    if man == "euclidean":
        return -(-x.numel() // 256), 256
    return x.shape[0], x.shape[1]


def _place(tensors, dev=lambda t, role: t.cuda()):
    """Host tensors -> [(man, X, G, [S])] on the device."""
    return [t if t is EMPTY else (t[0], dev(t[1], "p"), dev(t[2], "g"), [dev(s, "s") for s in t[3]]) for t in tensors]


def _descs(placed):
    c = _C()
    arr = (c.OptimTensor * max(len(placed), 1))()
    for d, (man, X, G, S) in zip(arr, placed):
        if man == "empty":
            d.dim, d.manifold = 1, 0                               # no rows: every pointer NULL
            continue
        d.rows, d.dim = _plan(man, X)
        d.param, d.grad, d.numel, d.manifold = X.data_ptr(), G.data_ptr(), X.numel(), MAN_ID[man]
        if S:
            d.state0 = S[0].data_ptr()
        if len(S) == 2:
            d.state1 = S[1].data_ptr()
    return arr


def _call(rule, arr, n, step, lr, wd, cfg, step_dev=None, lr_dev=None, stab=STAB):
    c = _C()
    if rule == "adam":
        return c.lib.hypad_optim_group_adam(arr, n, c.ptr(step_dev), step, c.ptr(lr_dev), lr, *cfg, wd, stab, c.stream())
    mu, damp, nest = cfg
    return c.lib.hypad_optim_group_sgd(arr, n, c.ptr(step_dev), step, c.ptr(lr_dev), lr, mu, damp, wd, int(nest), stab, c.stream())


def _gpu(rule, tensors, step, lr, wd, cfg, dev=None, **kw):
    """One grouped launch through the C ABI -> the placed list (updated in place)."""
    placed = _place(tensors, dev) if dev else _place(tensors)
    _C().check(_call(rule, _descs(placed), len(placed), step, lr, wd, cfg, **kw), f"grouped {rule}")
    torch.cuda.synchronize()
    return placed


def _outputs(placed):
    return [[X.cpu(), *[s.cpu() for s in S]] for man, X, G, S in placed if man != "empty"]


def _check_against_the_restatement(cks, case, rule, tensors, placed, step, lr, wd, cfg):
    real = [t for t in tensors if t is not EMPTY]
    r64, r32 = (gref.group_step(rule, real, step, lr, cfg, wd, STAB, dtype=dt) for dt in (F64, F32))
    got = _outputs(placed)
    G = [p[2] for p in placed if p[0] != "empty"]
    for k, ((man, x, grad, st), a, b, c_, gdev) in enumerate(zip(real, got, r64, r32, G)):
        ck = Ck(f"{case} tensor {k} ({man} {tuple(x.shape)})")
        for name, u, v, w in zip(NAMES[rule], a[1:], b[1:], c_[1:]):
            ck.cmp(name, u, v, w)
        po = x.double()
        ck.cmp("step (p_new - p_old) / lr", (a[0].double() - po) / lr, (b[0] - po) / lr, (c_[0].double() - po) / lr)
        if man == "ball" and x.shape[0] >= 3:
            assert abs(float(b[0][1].norm()) - manual.MAXNORM_F32) < 1e-12, f"{ck.case}: the reference's rim row does not end on project's limit"
        if rule == "adam" and man != "euclidean":                  # a row of exp_avg_sq that came in uniform leaves uniform
            bad = torch.nonzero((a[2] != a[2][:, :1]).any(1))
            if len(bad):
                ck.failures.append(f"{ck.case}: row {int(bad[0])} of exp_avg_sq is not one value repeated")
        if not torch.equal(gdev.cpu(), grad):
            ck.failures.append(f"{ck.case}: the gradient was written to")
        cks.append(ck)


def _grid_rows():
    """Rows one pass of the grouped kernel's grid covers, from the source: wave_grid's cap on the blocks times the waves of a block."""
    src = open(os.path.join(ROOT, "hypad_amd", "csrc", "optim_group.hip")).read()
    threads = int(re.search(r"constexpr int THREADS = (\d+);", src).group(1))
    assert "constexpr int WAVES = THREADS / 64;" in src
    cap = re.search(r"b > (\d+) \? (\d+) :", src[src.index("inline int wave_grid"):])
    assert cap and cap.group(1) == cap.group(2)
    return int(cap.group(1)) * (threads // 64)


# ================================================================================================ 1. one grouped launch against fp64
@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_one_mixed_launch(rule, dim):
    """Every kind in one launch at D on the lane and element-per-lane edges; steps 1 / 2 / 10 / 1000 from given moments (10 and 1000
    stabilise), weight decay 0 and 0.1, Adam and SGD without momentum, with it, with dampening and in Nesterov's form."""
    g = torch.Generator().manual_seed(100 * dim + len(rule))
    cks = []
    for step in STEPS:
        for wd in WDS:
            for cfg in CFGS[rule]:
                tensors = _with_cfg(rule, cfg, _mixed(g, rule, dim))
                placed = _gpu(rule, tensors, step, LR, wd, cfg)
                _check_against_the_restatement(cks, f"{rule} D {dim} step {step} wd {wd:g} cfg {cfg}", rule, tensors, placed, step, LR, wd, cfg)
    _finish(cks, f"{rule} mixed list D {dim}")


def _cycle(g, rule, n, dim=20):
    kinds = (("ball", 3), ("sphere", 2), ("euclidean", 257), ("ball", 1), ("euclidean", 5), ("sphere", 1))
    return [_tensor(g, rule, man, k, dim, k) for man, k in (kinds[i % len(kinds)] for i in range(n))]


@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_list_lengths_empty_tensors_and_a_block_in_three_tensors(rule):
    """Lists of 1 and of 32 tensors; a tensor without rows (every pointer NULL) first, in the middle and last; and ball (2, 63),
    sphere (1, 20), plain of 300 elements: the sphere's one row is wave 2 of block 0, whose four waves sit in three tensors of different
    manifold and dim."""
    g = torch.Generator().manual_seed(43)
    cfg = CFGS[rule][-1]
    lists = {"1 tensor": _cycle(g, rule, 1), "32 tensors": _cycle(g, rule, GROUP_MAX)}
    some = _cycle(g, rule, 4)
    lists["empty first, in the middle and last"] = [EMPTY, some[0], some[1], EMPTY, EMPTY, some[2], some[3], EMPTY]
    lists["a block in three tensors"] = [_tensor(g, rule, "ball", 2, 63), _tensor(g, rule, "sphere", 1, 20), _tensor(g, rule, "euclidean", 0, 0, 300)]
    cks = []
    for what, tensors in lists.items():
        placed = _gpu(rule, tensors, 10, LR, WDS[1], cfg)
        _check_against_the_restatement(cks, f"{rule} {what}", rule, tensors, placed, 10, LR, WDS[1], cfg)
    # all tensors empty: nothing to launch
    assert _call(rule, _descs([EMPTY, EMPTY]), 2, 10, LR, WDS[1], cfg) == HYPAD_OK
    _finish(cks, f"{rule} list forms")


@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_one_launch_past_the_grid(rule):
    """The first tensor has one pass of the capped grid plus five rows of D = 20, two small tensors follow: the grid-stride walk wraps,
    and the waves that wrap land in all three."""
    rows = _grid_rows() + 5
    assert rows == 4 * 4096 + 5
    g = torch.Generator().manual_seed(47)
    cfg = CFGS[rule][-1]
    tensors = [_tensor(g, rule, "ball", rows, 20), _tensor(g, rule, "sphere", 3, 65), _tensor(g, rule, "euclidean", 0, 0, 513)]
    cks = []
    placed = _gpu(rule, tensors, 10, LR, WDS[1], cfg)
    _check_against_the_restatement(cks, f"{rule} rows {rows}", rule, tensors, placed, 10, LR, WDS[1], cfg)
    _finish(cks, f"{rule} past the grid")


def _fresh_params(g, n):
    """n parameters of all kinds for the optimiser classes, with gradients: [(man, host x, host grad)]."""
    return [(man, x, grad) for man, x, grad, _ in _cycle(g, "adam", n)]


def _param(x, man):
    from hypad_amd.hyperspace import hyrnn_nets as hn
    if man == "euclidean":
        return torch.nn.Parameter(x.cuda())
    return hn.ManifoldParameter(x.cuda(), manifold=hn.PoincareBall() if man == "ball" else hn.Sphere())


@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_thirty_three_parameters_take_two_launches(rule):
    """33 parameters through the optimiser class, fresh state, two steps: 32 in one launch and the last in a second."""
    from hypad_amd import optim
    g = torch.Generator().manual_seed(53)
    host = _fresh_params(g, GROUP_MAX + 1)
    grads2 = [torch.randn(x.shape, generator=g) for _, x, _ in host]
    params = [_param(x, man) for man, x, _ in host]
    mu = f32(0.9)
    if rule == "adam":
        opt = optim.RiemannianAdam(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WDS[1], stabilize=2, manifold_rows=True, capturable=True)
    else:
        opt = optim.RiemannianSGD(params, lr=LR, momentum=mu, weight_decay=WDS[1], stabilize=2, capturable=True)
    cfg = (B1, B2, EPS) if rule == "adam" else (mu, 0.0, False)
    refs = {}
    for dt in (F64, F32):
        cur = [(man, x.to(dt), None, [torch.zeros_like(x, dtype=dt)] * 2 if rule == "adam" else [gr.to(dt)]) for man, x, gr in host]
        for t, grads in enumerate(([gr for _, _, gr in host], grads2), 1):
            out = gref.group_step(rule, [(man, x, gr.to(dt), st) for (man, x, _, st), gr in zip(cur, grads)], t, LR, cfg, WDS[1], 2)
            cur = [(man, o[0], None, list(o[1:])) for (man, _, _, _), o in zip(cur, out)]
        refs[dt] = cur
    for grads in ([gr for _, _, gr in host], grads2):
        for p, gr in zip(params, grads):
            p.grad = gr.cuda()
        opt.step()
    assert int(opt.param_groups[0]["step"]) == 2
    cks = []
    for k, (p, (man, x, _), a, b) in enumerate(zip(params, host, refs[F64], refs[F32])):
        ck = Ck(f"{rule} parameter {k} ({man} {tuple(x.shape)})")
        po = x.double()
        ck.cmp("(p_2 - p_0) / (2 lr)", (p.detach().double().cpu() - po) / (2 * LR), (a[1] - po) / (2 * LR), (b[1].double() - po) / (2 * LR), steps=2)
        for name, u, v in zip(NAMES[rule], a[3], b[3]):
            ck.cmp(name, opt.state[p][name], u, v, steps=2)
        assert opt.state[p]["step"] is opt.param_groups[0]["step"]
        cks.append(ck)
    _finish(cks, f"{rule} 33 parameters")


# ================================================================================================ 2. by value and from the device
@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_step_and_lr_from_the_device_give_the_bits_of_the_values(rule):
    g = torch.Generator().manual_seed(59)
    tensors = _mixed(g, rule, 65)
    cfg = CFGS[rule][-1]
    for step in (1, 9, 10):                                        # 10 stabilises
        want = _outputs(_gpu(rule, tensors, step, LR, WDS[1], cfg))
        sd, ld = torch.tensor([step], dtype=torch.int32, device="cuda"), torch.tensor([LR], device="cuda")
        for kw in (dict(step_dev=sd), dict(lr_dev=ld), dict(step_dev=sd, lr_dev=ld)):
            # (the by-value arguments that the device ones override are given other values)
            got = _outputs(_gpu(rule, tensors, 7 if "step_dev" in kw else step, 0.5 if "lr_dev" in kw else LR, WDS[1], cfg, **kw))
            for k, (a, b) in enumerate(zip(got, want)):
                assert all(torch.equal(u, v) for u, v in zip(a, b)), f"{rule} step {step} {sorted(kw)}: tensor {k} differs from the by-value call"
        assert int(sd) == step and float(ld) == LR                 # read, not written
    c = _C()
    counter = torch.tensor([41], dtype=torch.int32, device="cuda")
    c.check(c.lib.hypad_optim_step_advance(c.ptr(counter), c.stream()))
    assert int(counter) == 42


# ================================================================================================ 3. a tensor does not see the list
@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_a_tensor_gets_the_bits_it_gets_alone_wherever_it_stands(rule):
    g = torch.Generator().manual_seed(61)
    cfg = CFGS[rule][-1]
    fill = _cycle(g, rule, GROUP_MAX - 1)
    for probe in (_tensor(g, rule, "ball", 6, 20), _tensor(g, rule, "sphere", 5, 256), _tensor(g, rule, "euclidean", 0, 0, 513),
                  _tensor(g, rule, "ball", 1, 63)):
        alone = _outputs(_gpu(rule, [probe], 10, LR, WDS[1], cfg))[0]
        for at in (0, 17, 31):
            got = _outputs(_gpu(rule, fill[:at] + [probe] + fill[at:], 10, LR, WDS[1], cfg))[at]
            assert all(torch.equal(a, b) for a, b in zip(got, alone)), f"{rule} {probe[0]} {tuple(probe[1].shape)}: the bits at index {at} differ"


# ================================================================================================ 4. in place, nothing else touched
@pytest.mark.parametrize("rule", ("adam", "sgd"))
def test_operands_at_storage_offset_one_between_guards(rule):
    """Every operand at storage offset 1; every written buffer between two sentinel words that stay; the gradients unchanged; the bits of
    the aligned call."""
    g = torch.Generator().manual_seed(67)
    cfg = CFGS[rule][-1]
    for dim in (63, 256):
        tensors = _mixed(g, rule, dim)
        want = _outputs(_gpu(rule, tensors, 10, LR, WDS[1], cfg))
        bufs = []

        def dev(t, role):
            if role == "g":
                return _at_offset(t.cuda(), 1)
            buf, v = _guarded(t.shape, 1)                          # (the sentinel in front is the buffer's word 0)
            v.copy_(t)
            bufs.append(buf)
            return v
        placed = _gpu(rule, tensors, 10, LR, WDS[1], cfg, dev=dev)
        assert len(bufs) == sum(1 + len(t[3]) for t in tensors)
        assert all(_guards_intact(buf, 1) for buf in bufs), f"{rule} D {dim}: a guard word around a written buffer changed"
        assert all(torch.equal(p[2].cpu(), t[2]) for p, t in zip(placed, tensors))
        for k, (a, b) in enumerate(zip(_outputs(placed), want)):
            assert all(torch.equal(u, v) for u, v in zip(a, b)), f"{rule} D {dim}: tensor {k} at storage offset 1 differs from the aligned call"


# ================================================================================================ 5. the captured training step
def _sets(in_dim, classes, rows=32):
    g = torch.Generator().manual_seed(71)
    return [(_ball_rows(g, rows, in_dim, edge=False, zero_row=False, radius=0.9).cuda(), torch.randint(0, classes, (rows,), generator=g).cuda())
            for _ in range(2)]


def _train_step(model, opt, x, y):
    opt.zero_grad(set_to_none=True)
    loss = torch.nn.functional.cross_entropy(model(x), y)
    loss.backward()
    opt.step()
    return loss.detach()


def _snapshot(model, opt):
    out = {}
    for name, p in model.named_parameters():
        out[name] = p.detach().clone()
        for k, v in opt.state[p].items():
            if k != "step":
                out[f"{name}.{k}"] = v.detach().clone()
    return out


def _run_eager(model, opt, sets, order):
    for i in order:
        _train_step(model, opt, *sets[i])
    torch.cuda.synchronize()
    return _snapshot(model, opt)


def _run_captured(model, opt, sets, order, warm=3, before_replay=None):
    """`warm` eager steps on the capture stream, then zero_grad / forward / loss / backward / step captured as one linear chain on one
    stream and replayed for the rest of `order`, the data copied into the static inputs, nothing synchronised in between.
    -> (snapshot, [loss of every replay])."""
    x, y = sets[order[0]][0].clone(), sets[order[0]][1].clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for k, i in enumerate(order[:warm]):
            if before_replay:
                before_replay(k)
            x.copy_(sets[i][0])
            y.copy_(sets[i][1])
            _train_step(model, opt, x, y)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        loss = _train_step(model, opt, x, y)
    losses = []
    for k, i in enumerate(order[warm:], warm):
        if before_replay:
            before_replay(k)
        x.copy_(sets[i][0])
        y.copy_(sets[i][1])
        graph.replay()
        losses.append(loss.clone())
    torch.cuda.synchronize()
    return _snapshot(model, opt), [float(v) for v in losses]


ORDER = (0, 1, 0, 1, 0, 1, 0, 1, 0)                                # three eager steps, then six replays: B, A, B, A, B, A


def _optimisers(which):
    from hypad_amd import optim
    if which == "radam":
        return lambda ps, cap: optim.RiemannianAdam(ps, lr=1e-2, stabilize=2, manifold_rows=True, capturable=cap)
    if which == "rsgd":
        return lambda ps, cap: optim.RiemannianSGD(ps, lr=1e-2, momentum=0.9, nesterov=True, stabilize=3, capturable=cap)
    return lambda ps, cap: optim.Adam(ps, lr=1e-2, capturable=cap)


def _head(which):
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(73)
    return (torch.nn.Linear(20, 6) if which == "adam" else hyrnn_nets.MobiusDist2Hyperplane(20, 6)).cuda()


@pytest.mark.parametrize("which", ("radam", "rsgd", "adam"))
def test_the_captured_training_step(which):
    """Nine steps, the last six as replays of one captured graph, are bit for bit nine eager steps of the same capturable optimiser;
    the counter reads 9.  stabilize = 2 (3 under SGD) makes the replays alternate between the stabilising and the plain branch, and every
    replay has another bias correction: a step number frozen at capture cannot pass.  Against the default optimiser -- per-parameter
    launches, the step by value -- under the rule with steps = 9 (module docstring: err32 = 0 there); optim.Adam on an nn.Linear also
    against torch.optim.Adam on the CPU in fp64, with its fp32 run as the yardstick."""
    make, sets = _optimisers(which), _sets(20, 6)
    runs = {}
    for name in ("captured", "eager", "default"):
        model = _head(which)                                       # (seeded: the same weights every time)
        opt = make(list(model.parameters()), name != "default")
        runs[name] = _run_captured(model, opt, sets, ORDER)[0] if name == "captured" else _run_eager(model, opt, sets, ORDER)
        if name != "default":
            counter = opt.param_groups[0]["step"]
            assert isinstance(counter, torch.Tensor) and counter.dtype == torch.int32 and int(counter) == 9
            assert all(opt.state[p]["step"] is counter for p in model.parameters())
        else:
            assert opt.param_groups[0]["step"] == 9
    assert set(runs["captured"]) == set(runs["eager"]) == set(runs["default"])
    for k, v in runs["captured"].items():
        assert torch.equal(v, runs["eager"][k]), f"{which}: {k} after three eager steps and six replays differs from nine eager steps"
    ck = Ck(f"{which}: capturable against default over 9 steps")
    for k, v in runs["eager"].items():
        ck.cmp(k, v, runs["default"][k], runs["default"][k], steps=9)
    cks = [ck]
    if which == "adam":
        refs = []
        for dt in (F64, F32):
            model = _head(which).cpu().to(dt)
            opt = torch.optim.Adam(model.parameters(), lr=1e-2)
            for i in ORDER:
                _train_step(model, opt, sets[i][0].cpu().to(dt), sets[i][1].cpu())
            refs.append(_snapshot(model, opt))
        ck = Ck("adam: capturable against torch.optim.Adam over 9 steps")
        for k, v in runs["eager"].items():
            ck.cmp(k, v, refs[0][k], refs[1][k], steps=9)
        cks.append(ck)
    _finish(cks, f"{which} nine training steps")


# ================================================================================================ 6. a schedule through a captured step
def test_a_schedule_drives_a_captured_step():
    """lr as a one-element device tensor, refilled before every step: the replays take the value of their turn, bit for bit what eager
    steps of the capturable optimiser take with the same values given as floats."""
    from hypad_amd import optim
    sets = _sets(20, 6)
    lrs = [f32(v) for v in (1e-2, 2e-2, 5e-3, 3e-2, 1e-3, 8e-3, 2.5e-2, 4e-3, 1.5e-2)]
    model = _head("radam")
    lr = torch.tensor([lrs[0]], device="cuda")
    opt = optim.RiemannianAdam(model.parameters(), lr=lr, stabilize=2, manifold_rows=True, capturable=True)
    got, _ = _run_captured(model, opt, sets, ORDER, before_replay=lambda k: lr.fill_(lrs[k]))
    assert opt.param_groups[0]["lr"] is lr and int(opt.param_groups[0]["step"]) == 9
    model = _head("radam")
    opt = optim.RiemannianAdam(model.parameters(), lr=lrs[0], stabilize=2, manifold_rows=True, capturable=True)
    for k, i in enumerate(ORDER):
        opt.param_groups[0]["lr"] = lrs[k]
        _train_step(model, opt, *sets[i])
    want = _snapshot(model, opt)
    for k, v in got.items():
        assert torch.equal(v, want[k]), f"{k} under the captured schedule differs from eager steps with the same learning rates"
    # a default optimiser refuses the tensor
    opt = optim.RiemannianAdam(model.parameters(), lr=lr, manifold_rows=True)
    with pytest.raises(TypeError, match="capturable=True"):
        opt.step()


# ================================================================================================ 7. the sequence classifier
class _SeqClassifier(torch.nn.Module):
    """mobius_gru_loop (T = 3, 9 rows, 7 -> 5) -> MobiusDist2Hyperplane(5, 4): six parameters, plain, ball and sphere."""

    def __init__(self):
        super().__init__()
        from hypad_amd.hyperspace import hyrnn_nets as hn
        g = torch.Generator().manual_seed(79)
        uni = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * 5 ** -0.5
        self.weight_ih, self.weight_hh = torch.nn.Parameter(uni(15, 7)), torch.nn.Parameter(uni(15, 5))
        self.bias = hn.ManifoldParameter(_ball_rows(g, 3, 5, edge=False, zero_row=False, radius=0.5), manifold=hn.PoincareBall())
        torch.manual_seed(79)
        self.head = hn.MobiusDist2Hyperplane(5, 4)
        self.register_buffer("h0", torch.zeros(9, 5))

    def forward(self, x):
        from hypad_amd.hyperspace import hyrnn_nets as hn
        _, last = hn.mobius_gru_loop(x, self.h0, self.weight_ih, self.weight_hh, self.bias, -1.0)
        return self.head(last)


def test_the_sequence_classifier_in_one_graph():
    from hypad_amd import optim
    g = torch.Generator().manual_seed(83)
    sets = [(0.5 * torch.randn(3, 9, 7, generator=g).cuda(), torch.randint(0, 4, (9,), generator=g).cuda())]
    order = (0,) * 6                                               # two eager steps, four replays, one data set: the loss falls
    make = lambda m: optim.RiemannianAdam(m.parameters(), lr=1e-2, stabilize=2, manifold_rows=True, capturable=True)
    model = _SeqClassifier().cuda()                                # (seeded: the same weights every time)
    got, losses = _run_captured(model, make(model), sets, order, warm=2)
    model = _SeqClassifier().cuda()
    opt = make(model)
    eager = [float(_train_step(model, opt, *sets[0])) for _ in order]
    want = _snapshot(model, opt)
    assert len(got) == 6 * 3 and set(got) == set(want)
    for k, v in got.items():
        assert torch.equal(v, want[k]), f"{k} after two eager steps and four replays differs from six eager steps"
    assert losses == eager[2:], (losses, eager)
    print(f"\nsequence classifier: loss {eager[0]:.5f} -> {losses[-1]:.5f}")
    assert all(np.isfinite(eager)) and losses[-1] < eager[0] and losses[-1] < losses[0]


# ================================================================================================ 8. refusals
def test_capturing_before_an_eager_step_is_refused():
    from hypad_amd import optim
    model, sets = _head("radam"), _sets(20, 6)
    for which in ("radam", "rsgd"):
        opt = _optimisers(which)(list(model.parameters()), True)
        opt.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(model(sets[0][0]), sets[0][1]).backward()
        before = [p.detach().clone() for p in model.parameters()]
        torch.cuda.synchronize()
        stream, graph, scratch = torch.cuda.Stream(), torch.cuda.CUDAGraph(), torch.zeros(4, device="cuda")
        with pytest.raises(RuntimeError, match="run one eager step before capturing"):
            with torch.cuda.graph(graph, stream=stream):
                scratch.add_(1.0)                                  # (something to capture: the graph is not empty)
                opt.step()
        torch.cuda.synchronize()
        assert all(torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))
        assert opt.param_groups[0].get("step", 0) == 0 and not any(opt.state[p] for p in model.parameters())
        del graph
    assert optim.RiemannianAdam(model.parameters()).param_groups[0]["capturable"] is False


def test_entry_points_refuse_bad_arguments_and_launch_nothing():
    c = _C()
    bufs = [torch.full((3 * 257,), SENTINEL, device="cuda") for _ in range(4)]

    def descs(n=1, rows=3, dim=100, man=1, numel=None, p=0, g=1, s0=2, s1=3):
        arr = (c.OptimTensor * max(n, 1))()
        for d in arr:
            d.rows, d.dim, d.manifold, d.numel = rows, dim, man, rows * dim if numel is None else numel
            d.param, d.grad, d.state0, d.state1 = (None if k is None else bufs[k].data_ptr() for k in (p, g, s0, s1))
        return arr
    acfg, scfg = CFGS["adam"][0], CFGS["sgd"][1]
    for rule, cfg in (("adam", acfg), ("sgd", scfg)):
        call = lambda n=1, step=1, step_dev=None, **kw: _call(rule, descs(n, **kw), n, step, LR, WDS[1], cfg, step_dev=step_dev)
        assert call(n=0) == HYPAD_EINVAL and call(n=GROUP_MAX + 1) == HYPAD_EINVAL and call(n=-1) == HYPAD_EINVAL
        assert call(step=0) == HYPAD_EINVAL and call(rows=-1) == HYPAD_EINVAL and call(dim=0) == HYPAD_EINVAL
        assert call(man=3) == HYPAD_EINVAL and call(man=-1) == HYPAD_EINVAL
        assert call(dim=257, rows=1) == HYPAD_EUNSUPPORTED and call(rows=2 ** 31 // 100 + 1) == HYPAD_EUNSUPPORTED
        assert call(p=None) == HYPAD_EINVAL and call(g=None) == HYPAD_EINVAL and call(s0=None) == HYPAD_EINVAL
        assert call(numel=299) == HYPAD_EINVAL and call(man=0, numel=200) == HYPAD_EINVAL and call(man=0, numel=301) == HYPAD_EINVAL
        assert call(rows=0, p=None, g=None, s0=None, s1=None) == HYPAD_OK
        assert _call(rule, None, 1, 1, LR, WDS[1], cfg) == HYPAD_EINVAL
    assert _call("adam", descs(s1=None), 1, 1, LR, WDS[1], acfg) == HYPAD_EINVAL
    assert _call("sgd", descs(), 1, 1, LR, WDS[1], CFGS["sgd"][0]) == HYPAD_EINVAL          # a buffer without momentum
    assert c.lib.hypad_optim_step_advance(None, c.stream()) == HYPAD_EINVAL
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in bufs)                                   # nothing ran
    # ... and these do run: a plain tensor with a short last row, and step 0 by value when the device counter is given
    one = torch.tensor([1], dtype=torch.int32, device="cuda")
    assert _call("sgd", descs(man=0, numel=201, s0=None), 1, 0, LR, WDS[1], CFGS["sgd"][0], step_dev=one) == HYPAD_OK
    torch.cuda.synchronize()
    assert not bool((bufs[0][:201] == SENTINEL).any()) and bool((bufs[0][201:] == SENTINEL).all())


# ================================================================================================ 9. the default path's bits
def test_the_default_steps_are_the_parents_entry_points():
    """Twelve steps of each class with ``capturable`` off against the entry points the classes have always called -- hypad_adam_step,
    hypad_radam_step, hypad_radam_rows_step, hypad_rsgd_rows_step -- called directly on copies: the option changed nothing when off."""
    from hypad_amd import optim
    c = _C()
    g = torch.Generator().manual_seed(89)
    host = [("euclidean", torch.randn(3, 100, generator=g) * 0.1), ("ball", _ball_rows(g, 1, 100, radius=0.9)[0]),
            ("ball", _ball_rows(g, 6, 20, edge=False, radius=0.9)), ("sphere", _data(g, "adam", "sphere", 5, 33)[0])]
    grads = [[torch.randn(x.shape, generator=g).cuda() for _, x in host] for _ in range(12)]
    wd, stab, mu = f32(1e-3), 5, f32(0.9)
    s = c.stream()

    def adam_direct(k, p, gr, st, t):
        return c.lib.hypad_adam_step(c.ptr(p), c.ptr(gr), c.ptr(st[0]), c.ptr(st[1]), p.numel(), t, LR, B1, B2, EPS, wd, s)

    def radam_direct(k, p, gr, st, t):
        man, x = host[k]
        if man == "euclidean" or x.dim() == 1:
            return c.lib.hypad_radam_step(c.ptr(p), c.ptr(gr), c.ptr(st[0]), c.ptr(st[1]), p.numel(), 0, p.numel() if man == "ball" else 0, t, LR, B1, B2,
                                          EPS, wd, stab, s)
        return c.lib.hypad_radam_rows_step(c.ptr(p), c.ptr(gr), c.ptr(st[0]), c.ptr(st[1]), x.shape[0], x.shape[1], MAN_ID[man], t, LR, B1, B2, EPS, wd,
                                           stab, s)

    def rsgd_direct(k, p, gr, st, t):
        man, x = host[k]
        kind, rows, dim = (MAN_ID[man], x.numel() // x.shape[-1], x.shape[-1]) if man != "euclidean" else optim._euclidean_rows(x.numel())
        return c.lib.hypad_rsgd_rows_step(c.ptr(p), c.ptr(gr), c.ptr(st[0]), rows, dim, kind, t, LR, mu, 0.0, wd, 1, stab, s)

    classes = (("Adam", lambda ps: optim.Adam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd), adam_direct, NAMES["adam"]),
               ("RiemannianAdam", lambda ps: optim.RiemannianAdam(ps, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd, stabilize=stab, manifold_rows=True),
                radam_direct, NAMES["adam"]),
               ("RiemannianSGD", lambda ps: optim.RiemannianSGD(ps, lr=LR, momentum=mu, weight_decay=wd, nesterov=True, stabilize=stab), rsgd_direct,
                NAMES["sgd"]))
    for name, make, direct, keys in classes:
        params = [_param(x, man) for man, x in host]
        opt = make(params)
        mine = [x.cuda() for _, x in host]
        states = [None] * len(host)
        for t, gs in enumerate(grads, 1):
            for k, (p, gr) in enumerate(zip(params, gs)):
                p.grad = gr
                if states[k] is None:
                    states[k] = [gr.clone()] if name == "RiemannianSGD" else [torch.zeros_like(mine[k]), torch.zeros_like(mine[k])]
                c.check(direct(k, mine[k], gr, states[k], t), name)
            opt.step()
        torch.cuda.synchronize()
        assert opt.param_groups[0]["step"] == 12 and opt.param_groups[0]["capturable"] is False
        for k, p in enumerate(params):
            assert torch.equal(p.detach(), mine[k]), f"{name}: parameter {k} differs from the direct calls"
            assert opt.state[p]["step"] == 12 and set(opt.state[p]) == {"step", *keys}
            for key, st in zip(keys, states[k]):
                assert torch.equal(opt.state[p][key], st), f"{name}: {key} of parameter {k} differs from the direct calls"


# ================================================================================================ 10. the state round trip
@pytest.mark.parametrize("which", ("radam", "rsgd", "adam"))
def test_state_round_trip_between_the_modes(which):
    """The state_dict of a capturable optimiser after three steps, loaded into a fresh capturable one -- whose fourth step has the bits
    of the original's -- and into a default one, whose fourth step agrees under the rule (err32 = 0: module docstring) and whose step is
    the integer 4."""
    make, sets = _optimisers(which), _sets(20, 6)
    model = _head(which)
    opt = make(list(model.parameters()), True)
    _run_eager(model, opt, sets, ORDER[:3])
    saved, weights = copy.deepcopy(opt.state_dict()), copy.deepcopy(model.state_dict())
    assert isinstance(saved["param_groups"][0]["step"], torch.Tensor) and int(saved["param_groups"][0]["step"]) == 3
    want = _run_eager(model, opt, sets, ORDER[3:4])
    got = {}
    for cap in (True, False):
        m2 = _head(which)
        m2.load_state_dict(weights)
        o2 = make(list(m2.parameters()), cap)
        o2.load_state_dict(copy.deepcopy(saved))
        group = o2.param_groups[0]
        assert group["capturable"] is cap and int(group["step"]) == 3 and isinstance(group["step"], torch.Tensor) == cap
        assert all(o2.state[p]["step"] is group["step"] for p in m2.parameters()) if cap else all(o2.state[p]["step"] == 3 for p in m2.parameters())
        got[cap] = _run_eager(m2, o2, sets, ORDER[3:4])
        assert int(group["step"]) == 4 and (cap or type(group["step"]) is int) and all(int(o2.state[p]["step"]) == 4 for p in m2.parameters())
    assert int(saved["param_groups"][0]["step"]) == 3              # the saved counter is its own tensor
    for k, v in want.items():
        assert torch.equal(got[True][k], v), f"{which}: {k} after the round trip differs from the original's fourth step"
    ck = Ck(f"{which}: the default optimiser's fourth step from a capturable state")
    for k, v in want.items():
        ck.cmp(k, got[False][k], v, v, steps=4)
    _finish([ck], f"{which} state round trip")
