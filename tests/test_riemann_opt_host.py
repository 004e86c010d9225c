"""CPU-only checks of the row-wise Riemannian optimiser steps: the restatement (tests/riemann_opt_ref.py) against the pinned ball / Adam
oracles, the sphere's invariants in fp64, the optimiser classes' plumbing on host tensors (no device call), and the C ABI and build."""
import os
import re

import pytest
import torch

import riemann_opt_ref as ref
from oracle import manual
from oracle import radam as oracle_radam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
LR, B1, B2, EPS, WD = 0.05, 0.9, 0.999, 1e-8, 0.1


def _ball(g, rows, dim, radius=0.9):
    a = torch.randn(rows, dim, generator=g, dtype=F64)
    return a / a.norm(dim=1, keepdim=True) * (torch.rand(rows, 1, generator=g, dtype=F64) * radius)


def _sphere(g, rows, dim):
    a = torch.randn(rows, dim, generator=g, dtype=F64)
    return a / a.norm(dim=1, keepdim=True)


# ================================================================================================ 1. ball / Adam against the oracle
def test_one_ball_row_under_adam_is_the_manual_oracle():
    """25 steps of one row, stabilize = 10 included, against oracle/manual.radam_ball_step (whose second moment is one scalar)."""
    g = torch.Generator().manual_seed(1)
    x = _ball(g, 1, 20)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    p, pm, pv = x[0].clone(), torch.zeros(20, dtype=F64), torch.zeros((), dtype=F64)
    for t in range(1, 26):
        grad = torch.randn(1, 20, generator=g, dtype=F64)
        x, m, v = ref.radam_ball_rows(x, grad, m, v, t, LR, B1, B2, EPS, WD, stabilize=10)
        p, pm, pv = manual.radam_ball_step(p, grad[0], pm, pv, t, LR, B1, B2, EPS, WD, stabilize=10)
        assert float((x[0] - p).abs().max()) < 1e-12 and float((m[0] - pm).abs().max()) < 1e-12, t
        assert float((v[0] - pv).abs().max()) < 1e-12 and bool((v[0] == v[0, 0]).all()), t


def test_ball_rows_under_adam_are_the_oracle_optimiser_on_each_row():
    """(5, 20) against oracle/radam.RiemannianAdam stepping every row as its own 1-D tagged parameter.  (In fp64 that oracle projects at
    1 - 1e-5, the restatement at the fp32 limit 1 - 4e-3: the rows stay inside radius 0.97 here, where neither projection acts --
    asserted.)"""
    g = torch.Generator().manual_seed(2)
    x = _ball(g, 5, 20)
    params = []
    for r in range(5):
        q = torch.nn.Parameter(x[r].clone())
        q.manifold = object()
        params.append(q)
    opt = oracle_radam.RiemannianAdam(params, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, stabilize=10)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(1, 26):
        grad = torch.randn(5, 20, generator=g, dtype=F64)
        for r, q in enumerate(params):
            q.grad = grad[r].clone()
        opt.step()
        x, m, v = ref.radam_ball_rows(x, grad, m, v, t, LR, B1, B2, EPS, WD, stabilize=10)
        assert float(x.norm(dim=1).max()) < 0.97
        for r, q in enumerate(params):
            st = opt.state[q]
            assert float((x[r] - q.detach()).abs().max()) < 1e-12, (t, r)
            assert float((m[r] - st["exp_avg"]).abs().max()) < 1e-12 and float((v[r] - st["exp_avg_sq"]).abs().max()) < 1e-12, (t, r)


# ================================================================================================ 2. the sphere's invariants
@pytest.mark.parametrize("rule", ("adam", "sgd", "sgd-nesterov"))
def test_sphere_steps_stay_on_the_sphere_with_a_tangent_state(rule):
    g = torch.Generator().manual_seed(3)
    x = _sphere(g, 5, 20)
    m, v, buf = torch.zeros_like(x), torch.zeros_like(x), None
    for t in range(1, 26):
        grad = torch.randn(5, 20, generator=g, dtype=F64)
        if rule == "adam":
            x, m, v = ref.radam_sphere_rows(x, grad, m, v, t, LR, B1, B2, EPS, WD, stabilize=10)
            w = m
        else:
            buf = grad.clone() if buf is None else buf
            x, buf = ref.rsgd_sphere_rows(x, grad, buf, t, LR, 0.9, 0.0 if rule == "sgd-nesterov" else 0.1, WD, rule == "sgd-nesterov", stabilize=10)
            w = buf
        assert float((x.norm(dim=1) - 1).abs().max()) < 1e-12, t
        assert float((x * w).sum(1).abs().max()) < 1e-12, t


def test_a_gradient_along_x_leaves_a_sphere_row_where_it_is():
    """The tangent space has no component along x: r = g - <x, g> x = c x (1 - |x|^2), at most 2.3e-16 |c| for a row normalised in fp64.
    SGD moves by lr |r|; Adam from fresh moments by lr |r| / (|r| + eps) <= lr * 2.3e-16 * 3 / 1e-8."""
    g = torch.Generator().manual_seed(4)
    x = _sphere(g, 5, 20)
    grad = x * torch.tensor([[3.0], [-2.0], [0.5], [1.0], [-1.0]], dtype=F64)
    y, _ = ref.rsgd_sphere_rows(x, grad, None, 1, LR)
    assert float((y - x).abs().max()) < 1e-15
    y, b = ref.rsgd_sphere_rows(x, grad, torch.zeros_like(x), 1, LR, 0.9)
    assert float((y - x).abs().max()) < 1e-15 and float(b.abs().max()) < 1e-15
    y, m, v = ref.radam_sphere_rows(x, grad, torch.zeros_like(x), torch.zeros_like(x), 1, LR, B1, B2, EPS)
    assert float((y - x).abs().max()) < LR * 1e-7 and float(m.abs().max()) < 1e-15
    one = torch.tensor([[1.0], [-1.0]], dtype=F64)                                   # D = 1: the tangent space is {0}
    y, m, v = ref.radam_sphere_rows(one, torch.tensor([[0.7], [0.3]], dtype=F64), torch.zeros_like(one), torch.zeros_like(one), 1, LR, B1, B2, EPS)
    assert torch.equal(y, one) and not bool(m.any()) and not bool(v.any())


def test_untagged_rows_under_sgd_follow_torch_sgd():
    """The identity maps: torch.optim.SGD's rule from the second step on.  (The first differs by geoopt's own start of the buffer -- a
    clone of the gradient that the same step then still multiplies and adds to, where torch takes the gradient as the buffer -- so the
    first step here is torch's, written out.)"""
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(4, 7, generator=g, dtype=F64)
    grads = [torch.randn(4, 7, generator=g, dtype=F64) for _ in range(6)]
    for nesterov, damp in ((False, 0.0), (True, 0.0)):
        q = torch.nn.Parameter(x0.clone())
        opt = torch.optim.SGD([q], lr=LR, momentum=0.9, dampening=damp, nesterov=nesterov)
        for gr in grads:
            q.grad = gr.clone()
            opt.step()
        x, buf = x0, None
        for t, gr in enumerate(grads, 1):
            if buf is None:
                x, buf = x - LR * ((gr + 0.9 * gr) if nesterov else gr), gr.clone()
            else:
                x, buf = ref.rsgd_euclidean_rows(x, gr, buf, t, LR, 0.9, damp, 0.0, nesterov)
        assert float((x - q.detach()).abs().max()) < 1e-12


# ================================================================================================ 3. plumbing on host tensors
def _layer():
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(0)
    layer = hyrnn_nets.MobiusDist2Hyperplane(8, 5)
    for prm in (layer.point, layer.tangent, layer.scale):
        prm.grad = torch.ones_like(prm)
    return layer


def test_the_default_still_refuses_and_manifold_rows_gets_to_the_device_check():
    from hypad_amd import _C, optim
    layer = _layer()
    for prm in (layer.point, layer.tangent):
        before = prm.detach().clone()
        with pytest.raises(NotImplementedError, match="Euclidean optimiser"):
            optim.RiemannianAdam([prm], lr=0.1).step()
        with pytest.raises(NotImplementedError, match="manifold_rows=True"):
            optim.RiemannianAdam([prm], lr=0.1, manifold_rows=False).step()
        for make in (lambda: optim.RiemannianAdam([prm], lr=0.1, manifold_rows=True), lambda: optim.RiemannianSGD([prm], lr=0.1, momentum=0.9),
                     lambda: optim.RiemannianSGD([prm], lr=0.1)):
            opt = make()
            with pytest.raises(_C.HypadError, match="must live on the GPU"):
                opt.step()
            assert torch.equal(prm.detach(), before)
    # untagged parameters and 1-D ball vectors as well
    from hypad_amd.hyperspace import hyrnn_nets
    bias = hyrnn_nets.MobiusLinear(8, 5, fp64_hyper=False).bias
    bias.grad = torch.ones_like(bias)
    for prm in (layer.scale, bias):
        for make in (lambda: optim.RiemannianAdam([prm], lr=0.1, manifold_rows=True), lambda: optim.RiemannianSGD([prm], lr=0.1)):
            with pytest.raises(_C.HypadError, match="must live on the GPU"):
                make().step()
    assert optim.RiemannianAdam([layer.point], manifold_rows=True).param_groups[0]["manifold_rows"] is True
    assert optim.RiemannianAdam([layer.point]).param_groups[0]["manifold_rows"] is False


def test_row_plans():
    from hypad_amd import _C, optim
    from hypad_amd.hyperspace import hyrnn_nets as hn
    ball, sphere = hn.PoincareBall(), hn.Sphere()
    mp = lambda shape, man: hn.ManifoldParameter(torch.zeros(shape), manifold=man)
    assert optim._manifold_rows(mp((5, 8), ball), "x") == (_C.MANIFOLD_BALL, 5, 8)
    assert optim._manifold_rows(mp((2, 3, 256), sphere), "x") == (_C.MANIFOLD_SPHERE, 6, 256)
    assert optim._manifold_rows(mp((7,), sphere), "x") == (_C.MANIFOLD_SPHERE, 1, 7)
    assert optim._manifold_rows(mp((7,), ball), "x") == (_C.MANIFOLD_BALL, 1, 7)           # (RiemannianSGD: one row)
    assert optim._manifold_rows(torch.nn.Parameter(torch.zeros(3, 4)), "x") is None
    assert optim._is_ball_vector(mp((7,), ball)) and not optim._is_ball_vector(mp((7,), sphere)) and not optim._is_ball_vector(mp((2, 7), ball))
    # an untagged parameter under RiemannianSGD: the widest row that divides its element count
    for n, want in ((1, (1, 1)), (12, (1, 12)), (256, (1, 256)), (512, (2, 256)), (514, (257, 2)), (257, (257, 1)), (128 * 300, (150, 256))):
        assert optim._euclidean_rows(n) == (_C.MANIFOLD_EUCLIDEAN,) + want, n


@pytest.mark.parametrize("which", ("adam", "sgd"))
def test_row_wise_refusals_raise_before_touching_a_device(which):
    from hypad_amd import optim
    from hypad_amd.hyperspace import hyrnn_nets as hn

    class Lorentz:
        pass

    mp = lambda data, man: hn.ManifoldParameter(data, manifold=man)
    cases = [mp(torch.zeros(5, 8), Lorentz()),                                       # an unknown manifold
             mp(torch.zeros(5, 8), hn.PoincareBall(c=0.5)),                          # a ball that is not the one at k = -1
             mp(torch.zeros(5, 257), hn.PoincareBall()), mp(torch.zeros(5, 257), hn.Sphere()),
             mp(torch.zeros(8, 5).t(), hn.Sphere()), mp(torch.zeros(5, 16)[:, ::2], hn.PoincareBall())]
    for prm in cases:                                                                # host tensors: a device call would raise HypadError
        prm.grad = torch.ones_like(prm)
        before = prm.detach().clone()
        opt = optim.RiemannianAdam([prm], lr=0.1, manifold_rows=True) if which == "adam" else optim.RiemannianSGD([prm], lr=0.1, momentum=0.9)
        with pytest.raises(NotImplementedError, match="supported"):
            opt.step()
        assert torch.equal(prm.detach(), before) and not opt.state[prm]


def test_riemannian_sgd_validates_its_hyper_parameters_as_torch_sgd_does():
    from hypad_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    for kw in (dict(lr=-0.1), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1e-3), dict(lr=0.1, nesterov=True),
               dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            optim.RiemannianSGD(p, **kw)
        if "lr" in kw and kw["lr"] > 0 and "nesterov" not in kw:
            with pytest.raises(ValueError):
                torch.optim.SGD(p, **kw)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        torch.optim.SGD(p, lr=0.1, nesterov=True)
    with pytest.raises(ValueError, match="Nesterov momentum requires a momentum and zero dampening"):
        optim.RiemannianSGD(p, lr=0.1, nesterov=True)
    opt = optim.RiemannianSGD(p, lr=0.1, momentum=0.9, nesterov=True, stabilize=10)
    want = dict(lr=0.1, momentum=0.9, dampening=0, weight_decay=0, nesterov=True, stabilize=10)
    assert all(opt.param_groups[0][k] == v for k, v in want.items())
    with pytest.raises(TypeError):
        optim.RiemannianSGD(p)                                                       # lr has no default


# ================================================================================================ 4. ABI and build
def _c_params(decl):
    return [a.strip() for a in decl.split(",")]


def test_entry_points_are_declared_bound_defined_and_built():
    from hypad_amd import _C, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    source = open(os.path.join(ROOT, "hypad_amd", "csrc", "riemann_opt.hip")).read()
    for name in ("hypad_radam_rows_step", "hypad_rsgd_rows_step"):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in include/hypad.h"
        defn = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*\{", source)
        assert defn, f"{name} is not defined in csrc/riemann_opt.hip"
        res, args = _C._SIGS[name]
        assert len(args) == len(_c_params(decl.group(1))) == len(_c_params(defn.group(1)))
        kinds = ["p" if "*" in a else "i64" if "int64_t" in a else "f" if a.startswith("float") else "p" if "hypad_stream_t" in a else "i"
                 for a in _c_params(decl.group(1))]
        import ctypes
        bound = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_float: "f", ctypes.c_int: "i"}
        assert kinds == [bound[a] for a in args], name
        assert hasattr(_C.lib, name)
    for name, val in (("EUCLIDEAN", 0), ("BALL", 1), ("SPHERE", 2)):
        assert re.search(r"HYPAD_MANIFOLD_%s\s*=\s*%d\b" % (name, val), header) and getattr(_C, "MANIFOLD_" + name) == val
    assert "riemann_opt.hip" in build.SOURCES and build.SOURCES.index("riemann_opt.hip") < build.SOURCES.index("tangent.hip")
    assert build.SOURCES[-2:] == ["tangent.hip", "dist2plane_matmul.hip"]


def test_the_kernels_are_one_templated_body_without_scratch():
    """One kernel body in the source; its five instantiations (ball / sphere x Adam, ball / sphere / plain x SGD) in the gfx950 code
    object, none with a spilled vector register or scratch."""
    from hypad_amd import build
    build.build()
    source = open(os.path.join(ROOT, "hypad_amd", "csrc", "riemann_opt.hip")).read()
    assert len(re.findall(r"__global__", source)) == 1
    ks = build.kernel_metadata(os.path.join(build.LIB_DIR, "riemann_opt.o"))
    assert len(ks) == 5 and all("riemann_rows_kernel" in k["name"] for k in ks), [k["name"] for k in ks]
    assert not [k["name"] for k in ks if k["vgpr_spill_count"] or k["private_segment_fixed_size"]]
