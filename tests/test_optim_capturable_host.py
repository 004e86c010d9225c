"""CPU-only checks of the capturable optimiser steps (csrc/optim_group.hip, hypad_amd.optim's ``capturable``): the C ABI and the build,
the code object, the option's plumbing on host tensors (no device call), the element-wise Adam restatement (tests/optim_group_ref.py)
against torch.optim.Adam, and the step conversion of load_state_dict."""
import ctypes
import os
import re

import pytest
import torch

import optim_group_ref as gref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
ENTRY_POINTS = ("hypad_optim_step_advance", "hypad_optim_group_adam", "hypad_optim_group_sgd")


def _c_params(decl):
    return [a.strip() for a in decl.split(",")]


# ================================================================================================ 1. ABI and build
def test_entry_points_are_declared_bound_defined_and_built():
    from hypad_amd import _C, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    source = open(os.path.join(ROOT, "hypad_amd", "csrc", "optim_group.hip")).read()
    assert "global: hypad_*;" in open(os.path.join(ROOT, "hypad_amd", "csrc", "exports.map")).read()
    for name in ENTRY_POINTS:
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert decl, f"{name} is not declared in include/hypad.h"
        defn = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*\{", source)
        assert defn, f"{name} is not defined in csrc/optim_group.hip"
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(_c_params(decl.group(1))) == len(_c_params(defn.group(1)))
        kinds = ["p" if "*" in a else "i64" if "int64_t" in a else "f" if a.startswith("float") else "p" if "hypad_stream_t" in a else "i"
                 for a in _c_params(decl.group(1))]
        bound = {ctypes.c_void_p: "p", ctypes.c_int64: "i64", ctypes.c_float: "f", ctypes.c_int: "i"}
        assert kinds == [bound[a] for a in args], name
        assert name in _C.EXPORTS and hasattr(_C.lib, name)
    assert re.search(r"#define\s+HYPAD_OPTIM_GROUP_MAX\s+32\b", header) and _C.OPTIM_GROUP_MAX == 32
    assert re.search(r"#define\s+HYPAD_ABI_VERSION\s+7\b", header) and _C.ABI_VERSION == 7


def test_the_descriptor_is_bound_field_by_field():
    from hypad_amd import _C
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    body = re.search(r"typedef struct hypad_optim_tensor \{(.*?)\} hypad_optim_tensor;", header, flags=re.S).group(1)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    kind = lambda f: ctypes.c_void_p if "*" in f else ctypes.c_int64 if f.startswith("int64_t") else ctypes.c_int
    assert [(f.split()[-1].lstrip("*"), kind(f)) for f in fields] == list(_C.OptimTensor._fields_)
    assert ctypes.sizeof(_C.OptimTensor) == 56


def test_the_source_list_orders_as_stated():
    from hypad_amd import build
    assert "optim_group.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "optim_group.hip"))
    assert build.SOURCES.index("riemann_opt.hip") < build.SOURCES.index("optim_group.hip") < build.SOURCES.index("tangent.hip")
    assert build.SOURCES[-2:] == ["tangent.hip", "dist2plane_matmul.hip"]
    # both files take the manifolds and rules from one header
    for src in ("riemann_opt.hip", "optim_group.hip"):
        assert '#include "riemann_rules.h"' in open(os.path.join(build.CSRC, src)).read()
    rules = open(os.path.join(build.CSRC, "riemann_rules.h")).read()
    assert all(f"struct {s} " in rules for s in ("Ball", "SphereM", "Euclid", "AdamRule", "SgdRule"))


def test_the_kernels_have_no_spill_and_no_scratch():
    """The grouped kernel once per rule and the counter's kernel; the descriptors are held to the kernel-argument limit at compile time."""
    from hypad_amd import build
    build.build()
    source = open(os.path.join(ROOT, "hypad_amd", "csrc", "optim_group.hip")).read()
    assert len(re.findall(r"__global__", source)) == 2 and "static_assert(sizeof(Group)" in source
    ks = build.kernel_metadata(os.path.join(build.LIB_DIR, "optim_group.o"))
    names = sorted(k["name"] for k in ks)
    assert len(ks) == 3 and sum("optim_group_kernel" in n for n in names) == 2 and sum("advance_kernel" in n for n in names) == 1, names
    assert not [k["name"] for k in ks if k["vgpr_spill_count"] or k["sgpr_spill_count"] or k["private_segment_fixed_size"] or k["group_segment_fixed_size"]]
    assert all(k["vgpr_count"] <= 128 for k in ks), [(k["name"], k["vgpr_count"]) for k in ks]      # four waves per SIMD


# ================================================================================================ 2. plumbing on host tensors
def _layer():
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(0)
    layer = hyrnn_nets.MobiusDist2Hyperplane(8, 5)
    for prm in (layer.point, layer.tangent, layer.scale):
        prm.grad = torch.ones_like(prm)
    return layer


def _makers(params, **kw):
    from hypad_amd import optim
    return (lambda: optim.Adam(params, lr=0.1, **kw), lambda: optim.RiemannianAdam(params, lr=0.1, manifold_rows=True, **kw),
            lambda: optim.RiemannianSGD(params, lr=0.1, momentum=0.9, **kw))


def test_capturable_defaults_to_false():
    from hypad_amd import optim
    p = [torch.nn.Parameter(torch.zeros(3))]
    for make in _makers(p):
        opt = make()
        assert opt.param_groups[0]["capturable"] is False and opt.defaults["capturable"] is False
    for make in _makers(p, capturable=True):
        assert make().param_groups[0]["capturable"] is True
    opt = optim.Adam(p)
    opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(2))], capturable=True))       # per group
    assert [g["capturable"] for g in opt.param_groups] == [False, True]


@pytest.mark.parametrize("capturable", (False, True))
def test_a_host_tensor_reaches_the_device_check_and_stays_unchanged(capturable):
    from hypad_amd import _C
    layer = _layer()
    params = [layer.scale, layer.point, layer.tangent]
    before = [p.detach().clone() for p in params]
    for make in _makers(params, capturable=capturable):
        opt = make()
        with pytest.raises(_C.HypadError, match="must live on the GPU"):
            opt.step()
        assert all(torch.equal(p.detach(), b) for p, b in zip(params, before))
        if capturable:                                             # ... before any state or counter exists
            assert opt.param_groups[0].get("step", 0) == 0 and not any(opt.state[p] for p in params)


def test_every_refusal_comes_before_any_device_call():
    """Host tensors throughout: a device call would raise HypadError, not these."""
    from hypad_amd import optim
    from hypad_amd.hyperspace import hyrnn_nets as hn
    layer = _layer()
    ok = layer.scale
    mp = lambda data, man: hn.ManifoldParameter(data, manifold=man)
    # the refused parameter comes LAST: nothing before it may have been touched either
    for bad in (mp(torch.zeros(5, 257), hn.PoincareBall()), mp(torch.zeros(5, 8), hn.PoincareBall(c=0.5)), mp(torch.zeros(8, 5).t(), hn.Sphere()),
                mp(torch.zeros(257), hn.PoincareBall())):
        bad.grad = torch.ones_like(bad)
        for opt in (optim.RiemannianAdam([ok, bad], lr=0.1, manifold_rows=True, capturable=True),
                    optim.RiemannianSGD([ok, bad], lr=0.1, momentum=0.9, capturable=True)):
            with pytest.raises(NotImplementedError, match="supported"):
                opt.step()
            assert not opt.state[ok] and not opt.state[bad] and opt.param_groups[0].get("step", 0) == 0
    # a rank-1 ball vector longer than a row: refused with the range, with or without manifold_rows
    long = mp(torch.zeros(257), hn.PoincareBall())
    long.grad = torch.ones_like(long)
    for flag in (False, True):
        with pytest.raises(NotImplementedError, match="from 1 to 256"):
            optim.RiemannianAdam([long], lr=0.1, manifold_rows=flag, capturable=True).step()
    # tagged parameters still need manifold_rows under RiemannianAdam, with the message of the default step
    for prm in (layer.point, layer.tangent):
        with pytest.raises(NotImplementedError, match="manifold_rows=True"):
            optim.RiemannianAdam([prm], lr=0.1, capturable=True).step()
    # lr as a tensor: only a capturable step reads it
    for make in _makers([ok]):
        opt = make()
        opt.param_groups[0]["lr"] = torch.tensor([0.1])
        with pytest.raises(TypeError, match="capturable=True"):
            opt.step()
        assert not opt.state[ok] and opt.param_groups[0].get("step", 0) == 0


def test_row_plans_of_the_grouped_step():
    from hypad_amd import _C, optim
    from hypad_amd.hyperspace import hyrnn_nets as hn
    for n, rows in ((1, 1), (255, 1), (256, 1), (257, 2), (513, 3), (8191, 32)):       # 8191 is prime: still 256 to a row
        assert optim._plain_rows(n) == (_C.MANIFOLD_EUCLIDEAN, rows, 256), n
    mp = lambda shape, man: hn.ManifoldParameter(torch.zeros(shape), manifold=man)
    radam = lambda **kw: optim.RiemannianAdam([torch.nn.Parameter(torch.zeros(1))], **kw)
    group = lambda **kw: radam(**kw).param_groups[0]
    on, off = radam(manifold_rows=True), radam()
    assert on._kind(group(manifold_rows=True), mp((5, 8), hn.PoincareBall())) == (_C.MANIFOLD_BALL, 5, 8)
    assert on._kind(group(manifold_rows=True), mp((2, 3, 7), hn.Sphere())) == (_C.MANIFOLD_SPHERE, 6, 7)
    assert on._kind(group(manifold_rows=True), torch.nn.Parameter(torch.zeros(3, 100))) == (_C.MANIFOLD_EUCLIDEAN, 2, 256)
    for o, g in ((on, group(manifold_rows=True)), (off, group())):                   # MobiusLinear's bias: one ball row either way
        assert o._kind(g, mp((20,), hn.PoincareBall())) == (_C.MANIFOLD_BALL, 1, 20)
    assert off._kind(group(), torch.nn.Parameter(torch.zeros(300))) == (_C.MANIFOLD_EUCLIDEAN, 2, 256)
    adam = optim.Adam([torch.nn.Parameter(torch.zeros(1))])
    assert adam._kind(adam.param_groups[0], mp((5, 8), hn.PoincareBall())) == (_C.MANIFOLD_EUCLIDEAN, 1, 256)      # Adam knows no manifolds


# ================================================================================================ 3. the element-wise rule
@pytest.mark.parametrize("wd", (0.0, 0.1))
def test_the_elementwise_restatement_is_torch_adam(wd):
    g = torch.Generator().manual_seed(41)
    x = torch.randn(7, 13, generator=g, dtype=F64)
    q = torch.nn.Parameter(x.clone())
    opt = torch.optim.Adam([q], lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    m, v = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(1, 26):
        grad = torch.randn(7, 13, generator=g, dtype=F64)
        q.grad = grad.clone()
        opt.step()
        x, m, v = gref.adam_elementwise(x, grad, m, v, t, 0.05, 0.9, 0.999, 1e-8, wd)
        st = opt.state[q]
        assert float((x - q.detach()).abs().max()) < 1e-12, t
        assert float((m - st["exp_avg"]).abs().max()) < 1e-12 and float((v - st["exp_avg_sq"]).abs().max()) < 1e-12, t


# ================================================================================================ 4. the step of a state_dict
def test_step_conversion_between_the_modes():
    from hypad_amd import optim
    cpu = torch.device("cpu")
    t = optim._step_to_mode(7, True, cpu)
    assert isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.shape == (1,) and int(t) == 7
    assert optim._step_to_mode(t, False) == 7 and type(optim._step_to_mode(t, False)) is int
    assert optim._step_to_mode(torch.tensor(5.0), False) == 5 and optim._step_to_mode(9, False) == 9      # (torch's own float step)
    u = optim._step_to_mode(t, True, cpu)
    assert u is not t and u.dtype == torch.int32 and int(u) == 7
    assert optim._step_to_mode(3, True, None) == 3                # no device known yet: the first eager step makes the counter


@pytest.mark.parametrize("saved_as", ("int", "tensor"))
def test_load_state_dict_keeps_the_optimisers_own_mode(saved_as):
    """A saved step of either kind into a default optimiser on host tensors: the step is an int, ``capturable`` stays off whatever the
    saved group says, and the per-parameter entries follow the group's."""
    from hypad_amd import optim
    step = 3 if saved_as == "int" else torch.tensor([3], dtype=torch.int32)
    for cls, kw, keys in ((optim.Adam, {}, ("exp_avg", "exp_avg_sq")), (optim.RiemannianSGD, dict(lr=0.1, momentum=0.9), ("momentum_buffer",))):
        p = torch.nn.Parameter(torch.zeros(4))
        opt = cls([p], **kw)
        sd = opt.state_dict()
        sd["param_groups"][0].update(step=step, capturable=saved_as == "tensor")
        sd["state"] = {0: dict(step=step, **{k: torch.ones(4) for k in keys})}
        opt.load_state_dict(sd)
        group = opt.param_groups[0]
        assert group["capturable"] is False and group["step"] == 3 and type(group["step"]) is int
        assert opt.state[p]["step"] == 3 and type(opt.state[p]["step"]) is int and all(bool((opt.state[p][k] == 1).all()) for k in keys)
        # ... and into a capturable optimiser on host tensors: no device to count on, so an int until the first eager step
        cap = cls([torch.nn.Parameter(torch.zeros(4))], capturable=True, **kw)
        cap.load_state_dict(sd)
        assert cap.param_groups[0]["capturable"] is True and cap.param_groups[0]["step"] == 3
