"""PoincareBall(c).dist_matmul, weighted_midpoint, weighted_midpoint_bmm and hyperbolic_attention at any negative curvature, on the host:
the restatement of tests/curvature_mm_ref.py against the reference's own recorded outputs at k = -0.5 and k = -2
(tests/golden/curvature_mm.npz, written by tests/golden/gen_curvature_mm.py) and, at k = -1, against the restatements the k = -1 sweeps
use; the scaling identity away from the floors and the value on one; the C ABI's declarations, bindings and argument checks; and the
refusals of the methods -- which come before any device call, so they run here.

The bounds.  The generator asserts that the reference's fp32 run lies within 1e-6 of its own fp64 run on every recorded array, relative to
max(1, max|array|); the restatement is held to the fp32 records at the same 1e-6, run in fp64 and in fp32 (the rule of the other host
pins).  At k = -1 the two sides are the same arithmetic: 1e-12 in fp64.  The scaling identity f_c(x) = f_1(s x) / s moves every
operation's rounding: 1e-9 in fp64.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import curvature_mm_ref as mr
from test_tangent_maps_host import _err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND, SAME_BOUND, SCALING_BOUND = 1e-6, 1e-12, 1e-9
HYPAD_EINVAL, HYPAD_EUNSUPPORTED = -1, -3
CURVATURES = (0.5, 2.0)
BETA = 1.7                                                              # gen_attention.BETA
BMM_KINDS = ("softmax", "signed", "zerow")
# name: (reducedim, keepdim, weights, posweight, lincomb, coadd): gen_weighted_midpoint.REDUCE_CASES
REDUCE_CASES = {
    "r0_none": ([0], False, None, False, False, False),
    "r0_pos": ([0], False, "pos", False, False, False),
    "r0_signed": ([0], False, "signed", False, False, False),
    "all_pos": (None, False, "pos", False, False, False),
    "all_none_lincomb": (None, False, None, False, True, False),
    "r0_pos_keepdim": ([0], True, "pos", False, False, False),
    "r0_signed_posweight": ([0], False, "signed", True, False, False),
    "r0_signed_lincomb": ([0], False, "signed", False, True, False),
    "r0_signed_posweight_lincomb": ([0], False, "signed", True, True, False),
    "r0_signed_coadd": ([0], False, "signed", False, False, True),
    "r0_scalar_lincomb": ([0], False, "scalar", False, True, False),
}
NAMES = ("dist_matmul", "weighted_midpoint_bmm", "weighted_midpoint", "hyp_attention")
ENTRY_POINTS = tuple(f"hypad_ball_{n}_{d}" for n in NAMES for d in ("fwd", "bwd"))
SOURCES = dict(dist_matmul="dist.hip", weighted_midpoint_bmm="midpoint.hip", weighted_midpoint="midpoint.hip", hyp_attention="attention.hip")


def load_fixture(name="curvature_mm"):
    with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
        return {k: z[k] for k in z.files}


def cases(ops, k):
    """[(case, labels, the restatement of the leaves, operands, grad_output)] over operands named as the fixture names them."""
    out = [("dm", ("out", "grad_x", "grad_y"), lambda a, b: mr.dist_matmul_ref(a, b, k), (ops["dm_x"], ops["dm_y"]), ops["dm_grad_output"])]
    for kind in BMM_KINDS:
        for lincomb in (False, True):
            out.append((f"bmm_{kind}_lincomb{int(lincomb)}", ("out", "grad_xs", "grad_w"),
                        lambda x, w, lc=lincomb: mr.weighted_midpoint_bmm_ref(x, w, k, lincomb=lc), (ops["bmm_xs"], ops[f"bmm_w_{kind}"]),
                        ops["bmm_grad_output"]))
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in REDUCE_CASES.items():
        fn = (lambda x, w=None, a=(reducedim, keepdim, lincomb, posweight, coadd):
              mr.weighted_midpoint_ref(x, k, weights=w, reducedim=a[0], keepdim=a[1], lincomb=a[2], posweight=a[3], coadd=a[4]))
        out.append(("red_" + name, ("out", "grad_xs") + (() if wk is None else ("grad_w",)), fn,
                    (ops["red_xs"],) + (() if wk is None else (ops[f"red_w_{wk}"],)),
                    ops["red_grad_output_all" if reducedim is None else "red_grad_output_r0"]))
    for name, with_bias in (("attn_plain", False), ("attn_bias", True)):
        bias = torch.from_numpy(ops["attn_bias"].astype(np.float64)) if with_bias else None
        out.append((name, ("out", "grad_q", "grad_keys", "grad_values"),
                    lambda q, keys, values, b=bias: mr.hyperbolic_attention_ref(q, keys, values, k, BETA, b), (ops["q"], ops["keys"], ops["values"]),
                    ops["attn_grad_output"]))
    return out


def run(fn, operands, go, dt):
    leaves = [torch.from_numpy(a.astype(np.float64)).to(dt).requires_grad_(True) for a in operands]
    o = fn(*leaves)
    gs = torch.autograd.grad(o, leaves, torch.from_numpy(go.astype(np.float64)).to(dt).reshape(o.shape))
    return [o.detach()] + list(gs)


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("c", CURVATURES)
def test_restatement_meets_the_recorded_reference(c, dt):
    fx = load_fixture()
    pre = f"c{c:g}."
    assert all(v.dtype == np.float32 for v in fx.values())
    ops = {k[len(pre) + 3:]: v for k, v in fx.items() if k.startswith(pre + "in.")}
    todo = cases(ops, -c)
    assert len(todo) == 1 + 6 + 11 + 2
    assert len(fx) == 2 * (len(ops) + sum(len(t[1]) for t in todo))
    for name, labels, fn, operands, go in todo:
        for lab, got in zip(labels, run(fn, operands, go, dt)):
            want = fx[f"{pre}{name}.{lab}"]
            assert np.isfinite(want).all() and tuple(got.shape) == want.shape, (name, lab)
            err = _err(got, want)
            assert err <= BOUND, (name, lab, c, str(dt), err)


def test_fixture_holds_the_points_at_the_radius_of_their_ball():
    fx, k1 = load_fixture(), {}
    for f in ("dist", "weighted_midpoint", "attention"):
        k1.update(load_fixture(f))
    for c in CURVATURES:
        s = math.sqrt(c)
        for mine, theirs in (("dm_x", "dm_x"), ("dm_y", "dm_y"), ("bmm_xs", "bmm_xs"), ("red_xs", "red_xs"), ("q", "q"), ("keys", "keys"),
                             ("values", "values")):
            assert np.abs(fx[f"c{c:g}.in.{mine}"].astype(np.float64) * s - k1[theirs]).max() <= 1e-7, (c, mine)
        for mine, theirs in (("bmm_w_signed", "bmm_w_signed"), ("red_w_pos", "red_w_pos"), ("attn_bias", "bias"), ("dm_grad_output", "dm_grad_output")):
            assert np.array_equal(fx[f"c{c:g}.in.{mine}"], k1[theirs]), (c, mine)
        assert abs(np.linalg.norm(fx[f"c{c:g}.in.q"], axis=-1).max() * s - 0.9) < 1e-6 and np.isneginf(fx[f"c{c:g}.in.attn_bias"]).sum() == 1


def test_at_k_minus_one_it_is_the_restatements_of_the_k_minus_one_sweeps():
    import attention_ref
    import dist_ref
    import midpoint_ref
    t = lambda a: torch.from_numpy(a.astype(np.float64))
    d, m, a = load_fixture("dist"), load_fixture("weighted_midpoint"), load_fixture("attention")
    pairs = [(mr.dist_matmul_ref(t(d["dm_x"]), t(d["dm_y"]), -1.0), dist_ref.dist_matmul_ref(t(d["dm_x"]), t(d["dm_y"])))]
    for kind in BMM_KINDS:
        for lc in (False, True):
            xs, w = t(m["bmm_xs"]), t(m[f"bmm_w_{kind}"])
            pairs.append((mr.weighted_midpoint_bmm_ref(xs, w, -1.0, lincomb=lc), midpoint_ref.weighted_midpoint_bmm_ref(xs, w, lincomb=lc)))
    for name, (reducedim, keepdim, wk, posweight, lincomb, coadd) in REDUCE_CASES.items():
        w = None if wk is None else t(m[f"red_w_{wk}"])
        kw = dict(weights=w, reducedim=reducedim, keepdim=keepdim, lincomb=lincomb, posweight=posweight, coadd=coadd)
        pairs.append((mr.weighted_midpoint_ref(t(m["red_xs"]), -1.0, **kw), midpoint_ref.weighted_midpoint_ref(t(m["red_xs"]), **kw)))
    for bias in (None, t(a["bias"])):
        q, keys, values = t(a["q"]), t(a["keys"]), t(a["values"])
        pairs.append((mr.hyperbolic_attention_ref(q, keys, values, -1.0, BETA, bias), attention_ref.hyperbolic_attention_ref(q, keys, values, BETA, bias)))
    masked = torch.zeros(5, 7, dtype=torch.float64)
    masked[2] = -math.inf                                                 # a fully masked query: the origin on both sides
    q, keys, values = t(a["q"]), t(a["keys"]), t(a["values"])
    pairs.append((mr.hyperbolic_attention_ref(q, keys, values, -1.0, BETA, masked), attention_ref.hyperbolic_attention_ref(q, keys, values, BETA, masked)))
    assert not pairs[-1][0][:, 2].any()
    assert len(pairs) == 1 + 6 + 11 + 3
    for i, (got, want) in enumerate(pairs):
        assert got.shape == want.shape and bool(torch.isfinite(got).all()) and _err(got, want) <= SAME_BOUND, (i, _err(got, want))


def _ball(g, shape, s, lo=0.05, hi=0.9):
    x = torch.nn.functional.normalize(torch.randn(*shape, generator=g, dtype=torch.float64), dim=-1)
    return x * (torch.rand(*shape[:-1], 1, generator=g, dtype=torch.float64) * (hi - lo) + lo) / s


@pytest.mark.parametrize("c", [0.25, 2.0, 7.3, 100.0])
def test_scaling_identity_away_from_the_floors(c):
    """f_c(points, weights) = f_1(s points, weights) / s with beta -> beta / s, s = sqrt(c): in fp64 on outputs and on every operand
    gradient, on operands with no coincident pair and no all-zero row (there the floors 1e-15 sit on unscaled quantities and the identity
    does not hold: the next test)."""
    g = torch.Generator().manual_seed(int(c * 100))
    s = math.sqrt(c)
    x, y, xs, vals = _ball(g, (2, 5, 3), s), _ball(g, (2, 7, 3), s), _ball(g, (2, 7, 4), s), _ball(g, (2, 7, 4), s)
    rx = _ball(g, (6, 9, 5), s, hi=0.6)
    w = torch.randn(2, 5, 7, generator=g, dtype=torch.float64) / 2
    rw = torch.rand(6, 9, generator=g, dtype=torch.float64) * 2 - 1
    bias = torch.randn(2, 5, 7, generator=g, dtype=torch.float64)
    bias[1, 2, 5] = -math.inf
    todo = [(lambda k, f, a, b: f * mr.dist_matmul_ref(a, b.transpose(-1, -2), k), (x, y), (1, 1)),
            (lambda k, f, a, b: f * mr.weighted_midpoint_bmm_ref(a, b, k), (xs, w), (1, 0)),
            (lambda k, f, a, b: f * mr.weighted_midpoint_bmm_ref(a, b, k, lincomb=True), (xs, w), (1, 0)),
            (lambda k, f, a, b: f * mr.weighted_midpoint_ref(a, k, weights=b, reducedim=[0]), (rx, rw), (1, 0)),
            (lambda k, f, a, b: f * mr.weighted_midpoint_ref(a, k, weights=b, reducedim=[0], lincomb=True, posweight=True), (rx, rw), (1, 0)),
            (lambda k, f, a, b: f * mr.weighted_midpoint_ref(a, k, weights=b, reducedim=[0], coadd=True), (rx, rw), (1, 0)),
            (lambda k, f, q, kk, v: f * mr.hyperbolic_attention_ref(q, kk, v, k, BETA if k != -1.0 else BETA / s, bias), (x, y, vals), (1, 1, 1))]
    for i, (fn, ops, exps) in enumerate(todo):
        la = [t.clone().requires_grad_(True) for t in ops]
        lb = [t.clone().requires_grad_(True) for t in ops]
        oa = fn(-c, 1.0, *la)
        ob = fn(-1.0, 1.0 / s, *(s ** e * t for e, t in zip(exps, lb)))
        go = torch.randn(oa.shape, generator=g, dtype=torch.float64)
        ga, gb = torch.autograd.grad(oa, la, go), torch.autograd.grad(ob, lb, go)
        for j, (p, q) in enumerate(zip((oa.detach(),) + ga, (ob.detach(),) + gb)):
            assert bool(torch.isfinite(p).all()) and _err(p, q) <= SCALING_BOUND, (i, j, c, _err(p, q))


@pytest.mark.parametrize("c", [0.25, 1.0, 2.0, 100.0])
def test_a_coincident_pair_sits_on_the_unscaled_floor(c):
    """u = max(num / den, 1e-15) is clamped before the scaling by s: (2 / s) artanh(s sqrt(1e-15)) = 6.3e-8 for every c, where pure
    scaling would give 6.3e-8 / s; and nothing flows back through the clamp."""
    s = math.sqrt(c)
    x = (torch.tensor([[0.25, -0.5, 0.125], [0.0, 0.0, 0.0]], dtype=torch.float64) / 2 / max(s, 1.0)).requires_grad_(True)
    d = mr.dist_matmul_ref(x, x.detach().t().clone(), -c)
    want = 2 / s * math.atanh(s * math.sqrt(1e-15))
    assert abs(want - 6.3246e-8) < 1e-11
    assert abs(float(d.detach()[0, 0]) - want) <= 1e-6 * want and abs(float(d.detach()[1, 1]) - want) <= 1e-6 * want
    (gx,) = torch.autograd.grad(d[0, 0] + d[1, 1], x)
    assert not gx.any()
    if c != 1.0:
        scaled = mr.dist_matmul_ref(s * x.detach(), s * x.detach().t(), -1.0) / s
        assert abs(float(scaled[0, 0]) - want / s) <= 1e-6 * want and abs(float(scaled[0, 0]) - want) > 0.2 * want * abs(1 - 1 / s)


def _signatures():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    sigs = {}
    for m in re.finditer(r"\bint (hypad_\w+)\(([^)]*)\)\s*;", text):
        kinds = []
        for a in m.group(2).split(","):
            a = a.strip()
            kinds.append(ctypes.c_void_p if "*" in a or a.startswith("hypad_stream_t") else ctypes.c_int64 if a.startswith("int64_t") else
                         ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int if a.startswith("int ") else
                         ctypes.c_double if a.startswith("double ") else None)
        sigs[m.group(1)] = kinds
    return sigs


def test_header_declares_and_the_binding_binds_the_eight_entry_points():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    assert "docs/history/curvature_matmul.md" in text and "den = max(1 - 2 c xy + c^2 x2 y2, 1e-15)" in text
    assert os.path.exists(os.path.join(ROOT, "docs", "history", "curvature_matmul.md"))
    header = _signatures()
    from hypad_amd import _C
    assert _C.ABI_VERSION == 7 and _C.lib.hypad_abi_version() == 7          # new entry points, no changed one: the version stays
    assert len(ENTRY_POINTS) == 8
    for name in ENTRY_POINTS:
        source = open(os.path.join(ROOT, "hypad_amd", "csrc", SOURCES[name[len("hypad_ball_"):-4]])).read()
        assert name in header and f"int {name}(" in source, name
        res, args = _C._SIGS[name]
        assert res is ctypes.c_int and args == header[name] and None not in args, (name, args, header[name])
        assert name in _C.EXPORTS and getattr(_C.lib, name).argtypes == args, name
        k1 = header[name.replace("hypad_ball_", "hypad_")]                # the k = -1 argument list plus `double c` before the stream
        assert args == k1[:-1] + [ctypes.c_double, ctypes.c_void_p] and _C._SIGS[name.replace("hypad_ball_", "hypad_")][1] == k1, name
    for f in ("hypad_weighted_midpoint_bmm_workspace_bytes", "hypad_weighted_midpoint_workspace_bytes", "hypad_hyp_attention_workspace_bytes"):
        assert f in _C.EXPORTS and f.replace("hypad_", "hypad_ball_") not in _C.EXPORTS       # the existing ones serve both


def test_entry_points_check_c_then_their_sizes_before_any_hip_call():
    """Host pointers throughout, on a machine that may have no device: every call below is answered by the argument checks."""
    from hypad_amd import _C
    L = _C.lib
    buf = (ctypes.c_double * 4096)()
    p, n64, dbl, sz = ctypes.cast(buf, ctypes.c_void_p), ctypes.c_int64, ctypes.c_double, ctypes.c_size_t
    big = sz(1 << 30)

    def dm_f(c=0.5, batch=2, N=5, M=7, D=3, ops=(p, p, p)):
        return L.hypad_ball_dist_matmul_fwd(*ops, n64(batch), n64(N), n64(M), D, dbl(c), None)

    def dm_b(c=0.5, batch=2, N=5, M=7, D=3, ops=(p, p, p)):
        return L.hypad_ball_dist_matmul_bwd(*ops, p, p, n64(batch), n64(N), n64(M), D, dbl(c), None)

    def bmm_f(c=0.5, batch=2, N=5, M=7, D=3, ops=(p, p, p), flags=0):
        return L.hypad_ball_weighted_midpoint_bmm_fwd(*ops, p, n64(batch), n64(N), n64(M), D, flags, dbl(c), None)

    def bmm_b(c=0.5, batch=2, N=5, M=7, D=3, ops=(p, p, p), flags=0, ws=p, nbytes=big):
        return L.hypad_ball_weighted_midpoint_bmm_bwd(ops[0], ops[1], ops[2], p, p, p, ws, nbytes, n64(batch), n64(N), n64(M), D, flags, dbl(c), None)

    def red_f(c=0.5, M=6, R=9, D=5, ops=(p, p, p), wn=54, flags=0):
        return L.hypad_ball_weighted_midpoint_fwd(ops[0], ops[1], n64(wn), ops[2], p, p, big, n64(M), n64(R), D, flags, dbl(c), None)

    def red_b(c=0.5, M=6, R=9, D=5, ops=(p, p, p), wn=54, flags=0, ws=p, nbytes=big):
        return L.hypad_ball_weighted_midpoint_bwd(ops[0], ops[1], n64(wn), ops[2], p, p, p, ws, nbytes, n64(M), n64(R), D, flags, dbl(c), None)

    def at_f(c=0.5, batch=2, N=5, M=7, D=3, E=4, ops=(p, p, p), beta=1.0, stride=0, bias=None):
        return L.hypad_ball_hyp_attention_fwd(*ops, bias, n64(stride), dbl(beta), p, p, p, n64(batch), n64(N), n64(M), D, E, dbl(c), None)

    def at_b(c=0.5, batch=2, N=5, M=7, D=3, E=4, ops=(p, p, p), beta=1.0, stride=0, bias=None, ws=p, nbytes=big):
        return L.hypad_ball_hyp_attention_bwd(*ops, bias, n64(stride), dbl(beta), p, p, p, p, p, p, ws, nbytes, n64(batch), n64(N), n64(M), D, E, dbl(c),
                                              None)

    calls = (dm_f, dm_b, bmm_f, bmm_b, red_f, red_b, at_f, at_b)
    for call in calls:
        for c in (0.0, -1.0, float("nan"), float("inf"), -float("inf")):
            assert call(c=c) == HYPAD_EINVAL, (call.__name__, c)
        assert call(c=float("nan"), D=257) == HYPAD_EINVAL, call.__name__                 # c first: D = 257 alone is EUNSUPPORTED
        assert call(D=257) == HYPAD_EUNSUPPORTED and call(D=0) == HYPAD_EINVAL, call.__name__
        assert call(ops=(None, p, p)) == HYPAD_EINVAL, call.__name__
    for call in (dm_f, dm_b, bmm_f, bmm_b, at_f, at_b):
        assert call(N=-1) == HYPAD_EINVAL and call(batch=2 ** 20, N=2 ** 6, M=2 ** 6) == HYPAD_EUNSUPPORTED, call.__name__   # 2^32 pairs
    assert dm_f(batch=0, ops=(None, None, None)) == dm_f(N=0, ops=(None, p, None)) == 0 and dm_f(D=256, batch=0) == 0
    assert bmm_f(flags=8) == bmm_b(flags=8) == HYPAD_EINVAL and bmm_f(M=0) == HYPAD_EINVAL and bmm_f(N=0) == 0
    assert bmm_b(ws=None) == bmm_b(nbytes=sz(16)) == -2                                   # HYPAD_EWORKSPACE
    assert red_f(flags=8) == red_f(wn=5) == red_f(M=0) == HYPAD_EINVAL and red_f(R=0, wn=1) == 0 and red_b(nbytes=sz(16)) == -2
    assert at_f(D=129) == at_f(E=129) == at_b(D=129) == HYPAD_EUNSUPPORTED and at_f(D=128, E=128, batch=0) == 0
    assert at_f(beta=float("nan")) == at_b(beta=float("inf")) == at_f(M=0) == HYPAD_EINVAL           # the rules of beta; a midpoint of no points
    assert at_f(bias=p, stride=3) == at_b(bias=p, stride=3) == HYPAD_EINVAL and at_b(nbytes=sz(16)) == -2
    assert at_f(N=0, ops=(None, p, p)) == 0


_Q, _K, _V = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3), torch.zeros(2, 7, 4)
_W, _RX = torch.zeros(2, 5, 7), torch.zeros(6, 9, 5)
# method: (a supported call's operands, then keyword arguments)
_SUPPORTED = {
    "dist_matmul": ((_Q, _K.transpose(-1, -2)), {}),
    "weighted_midpoint": ((_RX,), dict(weights=torch.zeros(6, 9), reducedim=[0], lincomb=True)),
    "weighted_midpoint_bmm": ((_V, _W), dict(lincomb=True)),
    "hyperbolic_attention": ((_Q, _K, _V), dict(beta=1.7, bias=torch.zeros(5, 7))),
}


def test_every_method_refuses_a_bad_c_before_anything_else():
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    bad = {"dist_matmul": ((_Q.double(), _K),), "weighted_midpoint": ((torch.zeros(0, 5),),), "weighted_midpoint_bmm": ((_V, _Q),),
           "hyperbolic_attention": ((_Q, _K, _V), dict(beta=float("nan")))}
    for c in (0.0, -1.0, float("inf"), float("nan")):
        ball = PoincareBall(c)
        for name, (ops, kw) in _SUPPORTED.items():
            with pytest.raises(NotImplementedError, match="c = "):
                getattr(ball, name)(*ops, **kw)
            with pytest.raises(NotImplementedError, match="c = "):                # ... bad operands included
                getattr(ball, name)(*bad[name][0], **(bad[name][1] if len(bad[name]) > 1 else {}))
    ball = PoincareBall(0.5)
    ball.c = torch.tensor(0.5, requires_grad=True)                       # learnable curvature is not part of this
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(NotImplementedError, match="requires grad"):
            getattr(ball, name)(*ops, **kw)
    ball.c = torch.tensor([0.5, 2.0])
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(NotImplementedError, match="one value"):
            getattr(ball, name)(*ops, **kw)


@pytest.mark.parametrize("c", [0.5, 1.0, 7.3])
def test_supported_calls_get_as_far_as_the_device_and_bad_operands_do_not(c):
    """Host tensors throughout: a refusal that came after the first device call would fail here with 'must live on the GPU'."""
    from hypad_amd import _C
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    ball = PoincareBall(c)
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(_C.HypadError, match="GPU"):
            getattr(ball, name)(*ops, **kw)
    refused = lambda: pytest.raises(NotImplementedError, match="is not implemented")
    yT = _K.transpose(-1, -2)
    # dist_matmul: fp32, the batch dimensions equal or absent, D <= 256, fewer than 2^31 pairs
    for x, y in ((_Q.double(), yT), (_Q, yT.double()), (_Q, _K), (torch.zeros(3, 5, 3), yT), (torch.zeros(5, 257), torch.zeros(257, 7)),
                 (torch.zeros(3), torch.zeros(3, 7)), (torch.zeros(5, 0), torch.zeros(0, 7)),
                 (torch.zeros(1, 3).expand(2 ** 16, 3), torch.zeros(3, 1).expand(3, 2 ** 15))):
        with refused():
            ball.dist_matmul(x, y)
    for x, y in ((_Q[0], yT), (_Q, yT[0]), (torch.zeros(4, 2, 5, 3), torch.zeros(4, 2, 3, 7)), (torch.zeros(5, 256), torch.zeros(256, 7))):
        with pytest.raises(_C.HypadError, match="GPU"):
            ball.dist_matmul(x, y)
    # weighted_midpoint_bmm
    for xs, w in ((_V.double(), _W), (_V, _W.half()), (_V, _Q), (torch.zeros(3, 7, 4), _W), (torch.zeros(7, 257), torch.zeros(5, 7)),
                  (torch.zeros(4), torch.zeros(5, 4))):
        with refused():
            ball.weighted_midpoint_bmm(xs, w)
    for xs, w in ((_V[0], _W), (_V, _W[0]), (torch.zeros(7, 256), torch.zeros(5, 7))):
        with pytest.raises(_C.HypadError, match="GPU"):
            ball.weighted_midpoint_bmm(xs, w)
    # weighted_midpoint: the pooling form
    for a, kw in (((_RX.double(),), {}), ((_RX,), dict(dim=0)), ((_RX,), dict(reducedim=[2])), ((_RX,), dict(reducedim=[0, 0])),
                  ((_RX,), dict(weights=torch.zeros(9, 6))), ((_RX,), dict(weights=torch.zeros(6, 9).double())), ((torch.zeros(4, 257),), {}),
                  ((torch.zeros(()),), {})):
        with refused():
            ball.weighted_midpoint(*a, **kw)
    with pytest.raises(NotImplementedError, match="a midpoint of no points"):
        ball.weighted_midpoint(torch.zeros(0, 9, 5), reducedim=[0])
    for a, kw in (((_RX,), {}), ((_RX,), dict(reducedim=-2, keepdim=True, posweight=True, weights=torch.zeros(9))), ((_RX,), dict(weights=torch.zeros(1), coadd=True)),
                  ((torch.zeros(6, 0, 5),), dict(reducedim=[0]))):
        with pytest.raises(_C.HypadError, match="GPU"):
            ball.weighted_midpoint(*a, **kw)
    # attention: D and E <= 128, the rules of beta and bias, a midpoint of no points
    nograd = torch.zeros(5, 7, requires_grad=True)
    for a, kw in (((_Q.double(), _K, _V), {}), ((_Q, _K, torch.zeros(2, 6, 4)), {}), ((_Q, torch.zeros(2, 7, 4), _V), {}), ((torch.zeros(3, 5, 3), _K, _V), {}),
                  ((torch.zeros(5, 129), torch.zeros(7, 129), torch.zeros(7, 4)), {}), ((_Q, _K, torch.zeros(2, 7, 129)), {}),
                  ((_Q, torch.zeros(2, 0, 3), torch.zeros(2, 0, 4)), {}), ((_Q, _K, _V), dict(beta=float("inf"))), ((_Q, _K, _V), dict(beta=torch.ones(2))),
                  ((_Q, _K, _V), dict(beta=torch.ones(1, requires_grad=True))), ((_Q, _K, _V), dict(bias=nograd)),
                  ((_Q, _K, _V), dict(bias=torch.zeros(7, 5))), ((_Q, _K, _V), dict(bias=torch.zeros(5, 7).double())),
                  ((_Q, _K, _V), dict(bias=torch.zeros(3, 5, 7)))):
        with refused():
            ball.hyperbolic_attention(*a, **kw)
    for a, kw in (((_Q[0], _K, _V), {}), ((_Q, _K, _V), dict(beta=torch.tensor(0.3), bias=torch.zeros(2, 5, 7))),
                  ((torch.zeros(5, 128), torch.zeros(7, 128), torch.zeros(7, 128)), {}), ((torch.zeros(2, 0, 3), _K, _V), {})):
        with pytest.raises(_C.HypadError, match="GPU"):
            ball.hyperbolic_attention(*a, **kw)


def test_gmath_keeps_its_refusal_of_every_other_curvature():
    from hypad_amd.hyperspace import gmath
    for call in (lambda: gmath.dist_matmul(_Q, _K.transpose(-1, -2), -0.5), lambda: gmath.weighted_midpoint(_RX, -0.5),
                 lambda: gmath.weighted_midpoint_bmm(_V, _W, -2.0), lambda: gmath.hyperbolic_attention(_Q, _K, _V, -2.0)):
        with pytest.raises(NotImplementedError, match="curvature k = "):
            call()


def test_at_c_one_a_method_is_the_gmath_function(monkeypatch):
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    ball, seen = PoincareBall(1.0), []
    for name in _SUPPORTED:
        monkeypatch.setattr(gmath, name, lambda *a, _n=name, **kw: seen.append((_n, [v for v in a if isinstance(v, float)][:1])) or _n)
    for name, (ops, kw) in _SUPPORTED.items():
        assert getattr(ball, name)(*ops, **kw) == name
    assert seen == [(n, [-1.0]) for n in _SUPPORTED]                      # k = -1 is handed on, positionally as gmath takes it
    seen.clear()
    other = PoincareBall(0.5)
    for name, (ops, kw) in _SUPPORTED.items():
        with pytest.raises(Exception, match="GPU"):
            getattr(other, name)(*ops, **kw)
    assert seen == []                                                     # any other c does not go through gmath's function
    for name in _SUPPORTED:
        assert name in PoincareBall.__doc__ or name == "weighted_midpoint"
    assert "curvature_matmul.md" in PoincareBall.__doc__
