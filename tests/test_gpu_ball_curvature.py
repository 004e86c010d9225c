"""PoincareBall(c) on the GPU: every method, forward and backward, at curvatures other than -1 (hypad_ball_<name>_fwd / _bwd of
csrc/tangent.hip; hyperspace/ball.py runs them) against the plain-torch restatement of tests/curvature_ref.py -- which
tests/test_ball_curvature_host.py holds to the reference's own recorded outputs at k = -0.5 and k = -2 -- run in fp64 and in fp32, under
the rule of tests/sweep_common.py (``C * err32 + F`` with steps = 1; no tolerance of its own).

Curvatures: c = 0.5 and 2 on the recorded operands of tests/golden/curvature.npz, c = 0.01 and 100 on random data whose points lie at
radii up to 0.95 / sqrt(c).  Shapes: the launch edges are swept at k = -1 (tests/test_gpu_tangent_maps.py, tests/test_gpu_gyro_ops.py) and
the kernel templates are shared, so (1, 5), (5, 64), (7, 65) and (7, 256) for every function -- ball widths 1, 64 and 255 for the
projections -- and (4 * 4096 + 1, 3), one row past a pass of the largest grid, once per kernel template.  The special rows -- x == y, both
operands zero, points at (1 - 1e-3) / sqrt(c), a zero tangent, t = 0, -1 and 40 -- get a test of their own and do not set err32 for the
others.  The gradient of dist at rows that are equal element by element is 0 by the library's rule (hyperspace/gmath.dist), where
autograd of the restatement divides rounding noise by its own norm: those two rows of its gradients are held to 0, not to the restatement.
"""
import math

import numpy as np
import pytest
import torch

import curvature_ref as cr
from sweep_common import Ck, F, C, _at_offset, _guarded, _guards_intact, _leaf

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
SHAPES = [(1, 5), (5, 64), (7, 65), (7, 256)]
PROJ_WIDTHS = {5: 1, 64: 64, 65: 64, 256: 255}                 # the ball side of sproj / inv_sproj at each shape's D
ONE_PASS = 4 * 4096                                            # rows of one pass of the largest grid (4 waves a block, 4096 blocks)
PER_TEMPLATE = ("expmap0", "expmap", "gyration", "geodesic", "mobius_scalar_mul", "inner", "inv_sproj")
PER_ROW = ("dist", "dist0", "lambda_x", "norm", "inner")
TIMED = ("geodesic", "geodesic_unit", "mobius_scalar_mul")
FIRST_GENERATION = ("project", "expmap0", "logmap0", "mobius_add", "mobius_pointwise_mul", "mobius_scalar_mul", "dist", "dist0")
NAMES = tuple(cr.FUNCTIONS)


def _C():
    from hypad_amd import _C as c
    return c


def _ball(c):
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    return PoincareBall(c)


def _finish(cks):
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _report(what, cks):
    print(f"\nball curvature {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f}")


def _unit(g, rows, D):
    a = torch.randn(rows, D, generator=g, dtype=F64)
    return a / a.norm(dim=1, keepdim=True).clamp_min(1e-300)


def _data(c, rows, D, seed=0, radius=0.95):
    """fp32 operands under the names of curvature_ref.FUNCTIONS: points at radii up to ``radius`` / sqrt(c), one of them (from three rows
    on) at (1 - 1e-3) / sqrt(c), beyond project's limit; tangents, weights, t and r of order one; h = inv_sproj(y) computed in fp64."""
    g = torch.Generator().manual_seed(7919 * rows + 31 * D + seed)
    s = math.sqrt(c)
    pts = {k: _unit(g, rows, D) * torch.rand(rows, 1, generator=g, dtype=F64) * radius / s for k in ("x", "y", "a", "b")}
    if rows >= 3 and radius > 0.9:
        pts["x"][1] *= (1 - 1e-3) / s / pts["x"][1].norm()
    d = {k: v.float() for k, v in pts.items()}
    for k in ("u", "v", "grad"):
        d[k] = (_unit(g, rows, D) * torch.rand(rows, 1, generator=g, dtype=F64) * 1.5).float()
    d["w"] = torch.randn(rows, D, generator=g)
    d["t"] = (0.1 + 0.8 * torch.rand(rows, 1, generator=g, dtype=F64)).float()
    d["r"] = (torch.rand(rows, 1, generator=g, dtype=F64) * 3 - 1).float()
    d["h"] = cr.inv_sproj(d["y"].double(), -c).float()
    d["go"] = torch.randn(rows, D + 1, generator=g)
    return d


def _go(d, shape):
    """grad_out for a result of ``shape`` from the (rows, D + 1) draw of the data."""
    go = d["go"]
    return go[:, 0].reshape(shape) if len(shape) == go.dim() - 1 else go[:, :shape[-1]].reshape(shape)


def _operands(name, d):
    return [d[k] for k in cr.FUNCTIONS[name][1]]


def _refs(name, ops, go, k):
    """[out, grads...] of the restatement at curvature k in fp64 and fp32."""
    res = {}
    for dt in (F64, F32):
        leaves = [_leaf(t, dt) for t in ops]
        o = cr.FUNCTIONS[name][0](*leaves, k)
        res[dt] = [o.detach()] + list(torch.autograd.grad(o, leaves, go.to(dt)))
    return res


def _run(fn, ops, go, place=lambda t: t.cuda()):
    leaves = [place(t).requires_grad_(True) for t in ops]
    out = fn(*leaves)
    out.backward(go.cuda())
    return [out.detach()] + [t.grad for t in leaves]


def _check(ck, name, res, got, grad_rows=None):
    labels = ["out"] + ["grad_" + k for k in cr.FUNCTIONS[name][1]]
    for lab, t, r64, r32 in zip(labels, got, res[F64], res[F32]):
        assert t.shape == r64.shape, (ck.case, name, lab, t.shape, r64.shape)
        assert bool(torch.isfinite(t).all()), (ck.case, name, lab)
        mask = None
        if grad_rows is not None and lab != "out":
            mask = np.zeros(tuple(r64.shape), dtype=bool)
            mask[grad_rows] = True
        ck.cmp(f"{name} {lab}", t.cpu(), r64, r32, mask=mask)


def _case(c, name, d, tag, grad_rows=None):
    ops = _operands(name, d)
    shape = tuple(cr.FUNCTIONS[name][0](*(t.double() for t in ops), -c).shape)
    go = _go(d, shape)
    ck = Ck(f"{name} c={c:g} {tag}")
    got = _run(getattr(_ball(c), name), ops, go)
    _check(ck, name, _refs(name, ops, go, -c), got, grad_rows)
    return ck, got


# ================================================================================================ the sweep
@pytest.mark.parametrize("rows,D", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("c", [0.01, 100.0])
def test_every_method_forward_and_backward(c, rows, D):
    d, dp = _data(c, rows, D), _data(c, rows, PROJ_WIDTHS[D])
    cks = [_case(c, name, dp if name in ("sproj", "inv_sproj") else d, (rows, D))[0] for name in NAMES]
    _report((c, rows, D), cks)
    _finish(cks)


@pytest.mark.parametrize("c", [0.5, 2.0])
def test_recorded_operands_through_the_methods(c):
    """The operands of tests/golden/curvature.npz (the k = -1 generators' points divided by sqrt(c)) under the recorded grad_output."""
    from test_ball_curvature_host import CASES, grad_output, load_fixture
    fx = {k: torch.from_numpy(v) for k, v in load_fixture().items()}
    cks = []
    for name, (_, sname, keys, gk) in CASES.items():
        ops = [fx[f"c{c:g}.{sname}.{k}"] for k in keys]
        kw = dict(keepdim=True) if name == "inner" else {}
        fn = lambda *a, _n=name, _kw=kw: getattr(_ball(c), _n)(*a, **_kw)
        ref = lambda *a, _n=name, _kw=kw: cr.FUNCTIONS[_n][0](*a, -c, **_kw)
        shape = tuple(ref(*(t.double() for t in ops)).shape)
        go = grad_output(fx[f"c{c:g}.{sname}.{gk}"], shape)
        res = {}
        for dt in (F64, F32):
            leaves = [_leaf(t, dt) for t in ops]
            o = ref(*leaves)
            res[dt] = [o.detach()] + list(torch.autograd.grad(o, leaves, go.to(dt)))
        ck = Ck(f"{name} c={c:g} recorded")
        # the gyro set holds an x == y row, which dist never sees (its operands are the tan set's)
        _check(ck, name, res, _run(fn, ops, go))
        cks.append(ck)
    _report((c, "recorded"), cks)
    _finish(cks)


def test_one_row_past_a_grid_pass_once_per_kernel_template():
    c = 2.0
    d = _data(c, ONE_PASS + 1, 3)
    cks = [_case(c, name, d, (ONE_PASS + 1, 3))[0] for name in PER_TEMPLATE]
    _report((ONE_PASS + 1, 3), cks)
    _finish(cks)


def _special(c, D=5):
    """Row 0: x == y (and a == b); row 1: zero in both; rows 2 and 3: x and y at (1 - 1e-3) / sqrt(c); row 4: a zero tangent u; rows 5, 6,
    7: t = 0, -1 and 40; row 8 ordinary."""
    d = _data(c, 9, D, seed=5, radius=0.8)
    s = math.sqrt(c)
    x, y = d["x"].double(), d["y"].double()
    x[2] *= (1 - 1e-3) / s / x[2].norm()
    y[3] *= (1 - 1e-3) / s / y[3].norm()
    d["x"], d["y"] = x.float(), y.float()
    d["y"][0], d["b"][0] = d["x"][0], d["a"][0]
    for k in ("x", "y", "a", "b"):
        d[k][1] = 0.0
    d["u"][4] = 0.0
    d["t"][5], d["t"][6], d["t"][7] = 0.0, -1.0, 40.0
    d["r"][5], d["r"][6], d["r"][7] = 0.0, -1.0, 40.0
    d["h"] = cr.inv_sproj(d["y"].double(), -c).float()
    return d


@pytest.mark.parametrize("c", [0.5, 2.0])
def test_special_rows(c):
    d = _special(c)
    cks = []
    for name in NAMES:
        rows = list(range(2, 9)) if name == "dist" else None           # dist at equal rows: gradient 0 by rule (the module docstring)
        ck, got = _case(c, name, d, "special rows", rows)
        if name == "dist":
            assert float(got[0][:2].abs().max()) == 0.0 and all(float(g[:2].abs().max()) == 0.0 for g in got[1:])
        cks.append(ck)
    ball = _ball(c)
    x, y, t = d["x"].cuda(), d["y"].cuda(), d["t"].cuda()
    assert float(ball.logmap(x, y)[:2].abs().max()) <= 1e-7 / math.sqrt(c)          # log_x(x) = 0 up to the rounding of (-x) (+) x
    assert float((ball.geodesic(t, x, y)[:2] - x[:2]).abs().max()) <= 1e-7 / math.sqrt(c)
    on_rim = ball.geodesic_unit(t, x, d["u"].cuda())[7].double().norm() * math.sqrt(c)
    assert abs(float(on_rim) - 1.0) <= 1e-6                                          # the tanh clamp holds at t sqrt(c) / 2 >= 14
    _report((c, "special rows"), cks)
    _finish(cks)


# ================================================================================================ the entry points, called directly
def _raw(name, c, ops, go, offset=16, need=None, place=lambda t: t.cuda()):
    """hypad_ball_<name>_fwd / _bwd (c None: hypad_<name>_fwd / _bwd, the k = -1 entry points) on guarded buffers: [out, grads...], a
    gradient that ``need`` leaves out being None; asserts that every guard word is intact."""
    cc = _C()
    ops = [place(t.reshape(-1) if (name in TIMED and i == 0) else t).contiguous() for i, t in enumerate(ops)]
    rows_op = ops[1] if name in TIMED else ops[0]
    rows, width = rows_op.shape[0], rows_op.shape[1]
    dim = width - 1 if name == "sproj" else width
    out_shape = (rows,) if name in PER_ROW else (rows, width + (1 if name == "inv_sproj" else -1 if name == "sproj" else 0))
    need = [True] * len(ops) if need is None else need
    bufs = [_guarded(out_shape, offset)] + [(_guarded(tuple(t.shape), offset) if n else (None, None)) for t, n in zip(ops, need)]
    go = go.cuda().contiguous()
    assert tuple(go.shape) == out_shape
    pre = "hypad_" if c is None else "hypad_ball_"
    tail = ([rows] if name in TIMED else []) + ([] if c is None else [c]) + [cc.stream()]
    cc.check(getattr(cc.lib, f"{pre}{name}_fwd")(*map(cc.ptr, ops), cc.ptr(bufs[0][1]), rows, dim, *tail), name)
    cc.check(getattr(cc.lib, f"{pre}{name}_bwd")(*map(cc.ptr, ops), cc.ptr(go), *(cc.ptr(v) for _, v in bufs[1:]), rows, dim, *tail), name)
    torch.cuda.synchronize()
    for buf, v in bufs:
        assert buf is None or _guards_intact(buf, offset), (name, "guard words")
    return [None if v is None else v.clone() for _, v in bufs]


def _raw_case(name, d, c):
    ops = _operands(name, d)
    shape = tuple(cr.FUNCTIONS[name][0](*(t.double() for t in ops), -1.0 if c is None else -c).shape)
    return ops, _go(d, shape)


@pytest.mark.parametrize("name", NAMES)
def test_entry_point_at_c_one(name):
    """c = 1.0 multiplies by 1.0, which changes no bit: the 17 functions of tangent.hip return the bits of their k = -1 entry points.  The
    other eight have older k = -1 kernels of another arithmetic: they are held to the restatement at k = -1 under the rule."""
    d = _data(1.0, 7, 65, seed=3)
    ops, go = _raw_case(name, d, 1.0)
    got = _raw(name, 1.0, ops, go)
    if name not in FIRST_GENERATION:
        want = _raw(name, None, ops, go)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (name, i)
    ck = Ck(f"{name} entry point at c = 1")
    res = _refs(name, [t.reshape(-1, 1) if (name in TIMED and i == 0) else t for i, t in enumerate(ops)], go, -1.0)
    _check(ck, name, res, [g.reshape(r.shape) for g, r in zip(got, res[F64])])
    _finish([ck])


@pytest.mark.parametrize("name", NAMES)
def test_operand_handling_of_the_entry_points(name):
    """An operand at an unaligned storage offset gives the same bits; the guard words around every output stay intact (at an aligned and
    at an odd offset); a gradient that is not asked for is not written and leaves the bits of the others as they are."""
    c = 0.5
    d = _data(c, 5, 65 if name not in ("sproj", "inv_sproj") else 64, seed=11)
    ops, go = _raw_case(name, d, c)
    base = _raw(name, c, ops, go)
    moved = _raw(name, c, ops, go, offset=3, place=lambda t: _at_offset(t.cuda(), 1))
    for i, (a, b) in enumerate(zip(base, moved)):
        assert torch.equal(a, b), (name, "unaligned", i)
    for skip in range(len(ops)):
        need = [i != skip for i in range(len(ops))]
        part = _raw(name, c, ops, go, need=need)
        assert part[1 + skip] is None
        for i, (a, b) in enumerate(zip(base, part)):
            assert b is None or torch.equal(a, b), (name, "without gradient", skip, i)
    # the method gives the entry points' bits
    got = _run(getattr(_ball(c), name), ops, go)
    for i, (a, b) in enumerate(zip(base, got)):
        assert torch.equal(a.reshape(b.shape), b), (name, "method", i)


# ================================================================================================ the methods
def test_methods_at_c_one_are_gmath():
    from hypad_amd.hyperspace import gmath
    d = _data(1.0, 7, 65, seed=1)
    ball = _ball(1.0)
    for name in NAMES:
        ops = _operands(name, d)
        shape = tuple(cr.FUNCTIONS[name][0](*(t.double() for t in ops), -1.0).shape)
        go = _go(d, shape)
        got = _run(getattr(ball, name), ops, go)
        want = _run(lambda *a, _n=name: getattr(gmath, _n)(*a, k=-1.0), ops, go)
        for i, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), (name, i)
    x = d["x"].cuda()
    assert torch.equal(ball.antipode(x), -x) and torch.equal(_ball(0.5).antipode(x), -x)
    assert torch.equal(ball.transp(x, d["y"].cuda(), d["v"].cuda()), gmath.parallel_transport(x, d["y"].cuda(), d["v"].cuda(), k=-1.0))


def test_scaling_identity_at_c_two():
    """f_c(a_0, ...) = s^eo f_1(s^e0 a_0, ...): the method at c = 2 against the scaled c = 1 result (gmath's kernels), within the sum of the
    two sides' allowances under the rule.  Points at radii up to 0.5 / sqrt(c): the scaled operands are rounded to fp32 once more, 2^-24 of
    their size, which functions this far from the rim pass on without growing it beyond the rule's floor."""
    c, s = 2.0, math.sqrt(2.0)
    d = _data(c, 7, 65, seed=2, radius=0.5)
    failures = []
    for name in NAMES:
        exps, eo = cr.EXPONENTS[name]
        ops = _operands(name, d)
        scaled = [(t.double() * s ** e).float() for t, e in zip(ops, exps)]
        shape = tuple(cr.FUNCTIONS[name][0](*(t.double() for t in ops), -c).shape)
        go = _go(d, shape)
        got = _run(getattr(_ball(c), name), ops, go)
        one = _run(getattr(_ball(1.0), name), scaled, (go.double() * s ** eo).float())
        want = [one[0].double() * s ** eo] + [g.double() * s ** e for g, e in zip(one[1:], exps)]
        rc, r1 = _refs(name, ops, go, -c), _refs(name, scaled, (go.double() * s ** eo).float(), -1.0)
        for i, (a, b) in enumerate(zip(got, want)):
            f = s ** eo if i == 0 else s ** exps[i - 1]
            allow = 0.0
            for res, factor in ((rc, 1.0), (r1, f)):
                r64, r32 = res[F64][i].double(), res[F32][i].double()
                scale = max(1.0, float(r64.abs().max()))
                allow += factor * (C * float((r32 - r64).abs().max()) / scale + F) * scale
            err = float((a.double().cpu() - b.cpu()).abs().max())
            if not err <= allow:
                failures.append(f"{name} tensor {i}: |f_c - s^eo f_1| = {err:.3e} > {allow:.3e}")
    assert not failures, "\n".join(failures)


def test_capture_and_replay_give_the_eager_bits():
    """logmap -> transp0back at c = 0.5, forward and backward, captured once and replayed three times on new operand values."""
    c = 0.5
    ball = _ball(c)
    sets = [_data(c, 7, 65, seed=20 + i) for i in range(4)]
    x, y = (sets[0][k].cuda().requires_grad_(True) for k in ("x", "y"))
    go = _go(sets[0], (7, 65)).cuda()

    def step():
        x.grad = y.grad = None
        out = ball.transp0back(x, ball.logmap(x, y))
        out.backward(go)
        return out

    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        step()                                                          # the eager warm-up, on the capture stream
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):                        # one linear chain: nothing here forks a stream
        out = step()
    gx, gy = x.grad, y.grad
    for d in sets[1:]:
        with torch.no_grad():
            x.copy_(d["x"].cuda())
            y.copy_(d["y"].cuda())
        graph.replay()
        torch.cuda.synchronize()
        got = [out.clone(), gx.clone(), gy.clone()]
        ex, ey = (d[k].cuda().requires_grad_(True) for k in ("x", "y"))
        eager = ball.transp0back(ex, ball.logmap(ex, ey))
        eager.backward(go)
        for i, (a, b) in enumerate(zip(got, [eager.detach(), ex.grad, ey.grad])):
            assert torch.equal(a, b), i


def test_riemannian_gradient_descent_on_a_ball_of_another_radius():
    """p <- expmap(p, -lr egrad2rgrad(p, grad)) on dist(p, target).sum() at c = 0.5: the loss falls at every one of ten steps and every
    iterate stays inside the radius 1 / sqrt(c).  The Riemannian gradient of a distance has Riemannian norm 1, so a step moves every row
    lr along its geodesic towards the target: with every target further than the ten steps reach, the loss falls by rows * lr a step."""
    c, lr, rows = 0.5, 0.05, 16
    ball = _ball(c)
    g = torch.Generator().manual_seed(4)
    p = (_unit(g, rows, 8) * 0.6 / math.sqrt(c)).float().cuda()
    target = (_unit(g, rows, 8) * 0.7 / math.sqrt(c)).float().cuda()
    assert float(ball.dist(p, target).min()) > 10 * lr + 0.1
    losses = []
    for _ in range(10):
        p = p.detach().requires_grad_(True)
        loss = ball.dist(p, target).sum()
        (grad,) = torch.autograd.grad(loss, p)
        losses.append(float(loss.detach()))
        with torch.no_grad():
            p = ball.expmap(p, -lr * ball.egrad2rgrad(p, grad))
        assert float(p.norm(dim=-1).max()) < 1 / math.sqrt(c)
    losses.append(float(ball.dist(p, target).sum()))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs((losses[0] - losses[-1]) - 10 * rows * lr) <= 1e-3 * losses[0], losses
