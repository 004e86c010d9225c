"""Every calling form of the first-generation layer functions (the table: tests/layer_call_forms_cases.py).

The sweeps hold the kernels behind these functions to fp64 in the one form the package itself uses: 2-D contiguous fp32 operands, at least
one row, every operand requiring grad.  Here the Python wrappers are held to that form.  The canonical call of every entry is compared
once with its fp64 reference under the project's rule (sweep_common.Checker: C = 8, F = 2e-6).  Every other assertion is ``torch.equal``
against the same public call on equivalent canonical operands, or an exception type:

    ranks      row operands (D,), (10, D), (2, 5, D), (2, 1, 5, D) against the 2-D call on the flattened rows; shapes as the reference's
    views      each operand transposed, every second row of a taller buffer, a column window of a wider one, expanded from one row, and
               grad_outputs expanded from a scalar or transposed, against the call on .contiguous() clones; the buffers unchanged
    no rows    (0, D), (2, 0, D), (T, 0, in): empty fp32 results, empty row gradients, exact zeros for parameters, no HIP error left
    dtype      fp64 / fp16 / bf16 row operands against the call on x.float(); the leaf's gradient in the leaf's dtype
    twice      one tensor as both operands against two equal clones; the one gradient is the fp32 sum of the two
    single     each operand alone requiring grad, no_grad and inference_mode against the all-operands run
"""
import pytest
import torch

import layer_call_forms_cases as cf
from sweep_common import Checker

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
LEADS = [(), (10,), (2, 5), (2, 1, 5)]
_ENTRIES = {}


def _entry(name):
    if not _ENTRIES:
        _ENTRIES.update({e.name: e for e in cf.entries()})
    return _ENTRIES[name]


def _cuda(host):
    return {k: v.cuda() for k, v in host.items()}


def _same(what, got, want):
    """got and want ([outputs], {gradients}) hold the same bits (shapes may differ by a reshape of the leading dimensions)."""
    bad = []
    for i, (g, w) in enumerate(zip(got[0], want[0])):
        if g.dtype != w.dtype or g.numel() != w.numel() or not torch.equal(g.reshape(w.shape), w):
            bad.append(f"output {i} {tuple(g.shape)} {g.dtype}")
    assert set(got[1]) == set(want[1]), (what, sorted(got[1]), sorted(want[1]))
    for n, w in want[1].items():
        g = got[1][n]
        if g.dtype != w.dtype or g.numel() != w.numel() or not torch.equal(g.reshape(w.shape), w):
            bad.append(f"gradient of {n} {tuple(g.shape)} {g.dtype}")
    assert not bad, f"{what}: differs from the canonical call in " + ", ".join(bad)


def _finite(what, res):
    for t in [*res[0], *res[1].values()]:
        assert bool(torch.isfinite(t).all()), f"{what}: the canonical run is not finite (a NaN would compare unequal to itself)"


def test_the_table_is_the_one_named_here():
    es = cf.entries()
    assert [e.name for e in es] == cf.NAMES
    assert [e.name for e in es if e.grads] == cf.WITH_GRADS
    assert [e.name for e in es if e.grads and e.ranks == "flat"] == cf.FLAT
    assert [e.name for e in es if e.ranks == "refused"] == cf.REFUSED_RANKS
    assert [e.name for e in es if e.twice] == cf.TWICE


@pytest.mark.parametrize("name", cf.NAMES)
def test_canonical_call_meets_the_fp64_reference(name):
    e = _entry(name)
    host = e.build(1)
    outs, grads = cf.run(e, _cuda(host))
    (o64, g64), (o32, g32) = cf.reference(e, host, F64), cf.reference(e, host, F32)
    ck = Checker(name)
    for i, o in enumerate(outs):
        assert o.dtype == F32
        ck.cmp(f"output {i}", o, o64[i], o32[i], steps=cf.T if e.ranks is None else 1)
    for n in e.grads:
        ck.cmp(f"grad {n}", grads[n], g64[n], g32[n], steps=cf.T if e.ranks is None else 1)
    print(f"\nlayer call forms {name}: worst errgpu / allowance {ck.worst:.3f}")
    ck.done()


# ------------------------------------------------------------------------------------------------ 1. ranks
@pytest.mark.parametrize("name", cf.FLAT)
def test_leading_dimensions_give_the_bits_of_the_flattened_rows(name):
    e = _entry(name)
    for lead in LEADS:
        rows = 1
        for n in lead:
            rows *= n
        host = e.build(3, rows=rows, small=True)
        flat, shaped = _cuda(host), cf.with_lead(e, _cuda(host), lead)
        want, got = cf.run(e, flat), cf.run(e, shaped)
        _finite(name, want)
        ref = cf.reference(e, cf.with_lead(e, host, lead), F32)
        for i, (g, r) in enumerate(zip(got[0], ref[0])):
            assert g.shape == r.shape, f"{name}, lead {lead}: output {i} is {tuple(g.shape)}, the reference's is {tuple(r.shape)}"
        for n, r in ref[1].items():
            assert got[1][n].shape == r.shape, f"{name}, lead {lead}: the gradient of {n} is {tuple(got[1][n].shape)}, the reference's {tuple(r.shape)}"
        _same(f"{name}, lead {lead}", got, want)


@pytest.mark.parametrize("name", cf.REFUSED_RANKS)
def test_a_function_of_one_fixed_rank_refuses_another(name):
    from hypad_amd import _C
    e = _entry(name)
    host = e.build(3, rows=10)
    with pytest.raises((NotImplementedError, _C.HypadError)) as info:
        cf.run(e, cf.with_lead(e, _cuda(host), (2, 5)))
    assert "must live on the GPU" not in str(info.value) and "failed" not in str(info.value), info.value      # refused by the wrapper itself
    torch.cuda.synchronize()


def _add(x, y):
    from hypad_amd.hyperspace import gmath
    xl, yl = x.detach().requires_grad_(True), y.detach().requires_grad_(True)
    out = gmath.mobius_add(xl, yl)
    go = torch.linspace(-1, 1, out.numel(), device="cuda").reshape(out.shape)
    return (out.detach(), *torch.autograd.grad(out, [xl, yl], go))


@pytest.mark.parametrize("xs, ys", [((2, 5, 5), (5, 5)), ((1, 5), (10, 5)), ((2, 1, 5), (5, 5)), ((10, 5), (1, 5))])
def test_mobius_add_broadcasts_as_the_reference_does(xs, ys):
    """A y of fewer dimensions and more than one row, an x that broadcasts up to y, both at once, and a y of one row and all the
    dimensions of x: the result and both gradients are those of the call on the materialised broadcast, the gradient of a broadcast
    operand summed over the dimensions it was broadcast along (autograd's own sum, the expand's backward).  The y of one row and fewer
    dimensions, which the kernel broadcasts itself, is an entry of the table."""
    from oracle import gmath as og
    g = torch.Generator().manual_seed(5)
    x = cf._ball(g, torch.Size(xs).numel() // 5, 5).reshape(xs)
    y = cf._ball(g, torch.Size(ys).numel() // 5, 5, radius=0.5).reshape(ys)
    shape = torch.broadcast_shapes(xs, ys)
    assert og.mobius_add(x, y).shape == shape
    xd, yd = x.cuda(), y.cuda()
    out, gx, gy = _add(xd, yd)
    wout, wgx, wgy = _add(xd.expand(shape).contiguous(), yd.expand(shape).contiguous())
    assert out.shape == shape and gx.shape == xs and gy.shape == ys
    assert torch.equal(out, wout)
    assert torch.equal(gx, wgx.sum_to_size(xs)) and torch.equal(gy, wgy.sum_to_size(ys))


def test_mobius_add_names_both_shapes_when_they_do_not_broadcast():
    from hypad_amd import _C
    from hypad_amd.hyperspace import gmath
    with pytest.raises((NotImplementedError, _C.HypadError), match=r"\(2, 4, 8\).*\(3, 8\)"):
        gmath.mobius_add(torch.zeros(2, 4, 8, device="cuda"), torch.zeros(3, 8, device="cuda"))


# ------------------------------------------------------------------------------------------------ 2. views
def _views(t):
    """[(kind, the view, its whole buffer)]: the values of t (of its first row, for the expanded one) behind another layout."""
    out = []
    if t.dim() >= 2 and t.shape[-1] > 1 and t.shape[-2] > 1:
        base = t.transpose(-1, -2).contiguous()
        out.append(("transposed", base.transpose(-1, -2), base))
    tall = torch.randn(2 * t.shape[0], *t.shape[1:], device=t.device)
    tall[::2] = t
    out.append(("rows [::2]", tall[::2], tall))
    wide = torch.randn(*t.shape[:-1], t.shape[-1] + 2, device=t.device)
    wide[..., 1:-1] = t
    out.append(("columns [1:D+1]", wide[..., 1:t.shape[-1] + 1], wide))
    if t.shape[0] > 1:
        one = t[:1].clone()
        out.append(("expanded from one row", one.expand(t.shape), one))
    return out


@pytest.mark.parametrize("name", cf.NAMES)
def test_operands_that_are_views_give_the_bits_of_their_contiguous_clones(name):
    e = _entry(name)
    ops = _cuda(e.build(2))
    for n in e.operands(ops):
        for kind, view, base in _views(ops[n]):
            # (a view of another buffer: strided, of stride 0, or -- the window of a 1-D operand -- contiguous at an offset)
            assert view.shape == ops[n].shape, (n, kind)
            assert not view.is_contiguous() or view.untyped_storage().nbytes() != view.numel() * view.element_size(), (n, kind)
            before = base.clone()
            want = cf.run(e, {**ops, n: view.contiguous()})
            got = cf.run(e, {**ops, n: view})
            torch.cuda.synchronize()
            _finite(f"{name}, {n} {kind}", want)
            _same(f"{name}, {n} {kind}", got, want)
            assert torch.equal(base, before), f"{name}, {n} {kind}: the call changed the viewed buffer"


@pytest.mark.parametrize("name", cf.WITH_GRADS)
def test_grad_outputs_that_are_views_give_the_bits_of_their_contiguous_clones(name):
    """``out.sum().backward()`` hands the backward an expanded scalar; a loss on ``out.t()`` a transposed view."""
    e = _entry(name)
    ops = _cuda(e.build(2))
    scalar = torch.full((), 0.75, device="cuda")
    for kind in ("expanded scalar", "transposed"):
        gos, bases = [], []
        for g in e.gos:
            t = ops[g]
            if kind == "transposed" and t.dim() >= 2:
                base = t.transpose(-1, -2).contiguous()
                gos.append(base.transpose(-1, -2))
            else:
                base = scalar
                gos.append(scalar.expand(t.shape))
            bases.append(base)
        before = [b.clone() for b in bases]
        want = cf.run(e, ops, gos=[g.contiguous() for g in gos])
        got = cf.run(e, ops, gos=gos)
        torch.cuda.synchronize()
        _finite(f"{name}, grad_outputs {kind}", want)
        _same(f"{name}, grad_outputs {kind}", got, want)
        assert all(torch.equal(b, c) for b, c in zip(bases, before)), f"{name}, grad_outputs {kind}: the backward changed the viewed buffer"


# ------------------------------------------------------------------------------------------------ 3. no rows
@pytest.mark.parametrize("name", cf.NAMES)
def test_no_rows_give_empty_results_and_zero_parameter_gradients(name):
    e = _entry(name)
    host = e.build(4, rows=0)
    for lead in [(0,), (2, 0)] if e.ranks == "flat" else [(0,)]:
        hops = cf.with_lead(e, host, lead)
        ref = cf.reference(e, hops, F32)
        outs, grads = cf.run(e, _cuda(hops))
        torch.cuda.synchronize()
        for i, (o, r) in enumerate(zip(outs, ref[0])):
            assert o.dtype == F32 and o.shape == r.shape, f"{name}, rows {lead}: output {i} is {tuple(o.shape)} {o.dtype}, the reference's {tuple(r.shape)}"
            assert torch.equal(o.cpu(), r), f"{name}, rows {lead}: output {i} is not the reference's (empty, or 0 for a sum over no rows)"
        for n in e.grads:
            g = grads[n]
            assert g.shape == hops[n].shape and g.dtype == F32, (name, lead, n, tuple(g.shape), g.dtype)
            if n in e.rows:
                assert g.numel() == 0, (name, lead, n)
            else:
                assert bool((g == 0).all()), f"{name}, rows {lead}: the gradient of {n} over no rows is not all zero"
        assert float(torch.arange(4.0, device="cuda").sum()) == 6.0                     # no HIP error is left behind


# ------------------------------------------------------------------------------------------------ 4. dtype
@pytest.mark.parametrize("dt", [torch.float64, torch.float16, torch.bfloat16], ids=["fp64", "fp16", "bf16"])
@pytest.mark.parametrize("name", cf.NAMES)
def test_row_operands_of_another_dtype_are_cast_to_fp32(name, dt):
    e = _entry(name)
    ops = _cuda(e.build(5))
    cast = {**ops, **{n: ops[n].to(dt) for n in e.rows}}
    want = cf.run(e, {**ops, **{n: cast[n].float() for n in e.rows}})
    got = cf.run(e, cast)
    _finite(f"{name}, {dt}", want)
    for n in e.grads:
        if n in e.rows:
            assert got[1][n].dtype == dt, f"{name}: the gradient that arrives at the {dt} leaf {n} is {got[1][n].dtype}"
            want[1][n] = want[1][n].to(dt)
    _same(f"{name}, row operands in {dt}", got, want)
    assert all(o.dtype == F32 for o in got[0])


# ------------------------------------------------------------------------------------------------ 5. the same tensor twice
@pytest.mark.parametrize("name", cf.TWICE)
def test_one_tensor_as_both_operands(name):
    e = _entry(name)
    a, b = e.twice
    ops = _cuda(e.build(6))
    ops[b] = ops[a].clone()
    want = cf.run(e, ops)
    got = cf.run(e, ops, shared=(a, b))
    _finite(name, want)
    if e.grads:
        want[1][a] = want[1][a] + want[1].pop(b)
    _same(f"{name}, {b} is {a}", got, want)


# ------------------------------------------------------------------------------------------------ 6. one gradient at a time, and none
@pytest.mark.parametrize("name", cf.WITH_GRADS)
def test_each_operand_alone_requiring_grad_and_no_grad_at_all(name):
    e = _entry(name)
    ops = _cuda(e.build(7))
    full = cf.run(e, ops)
    _finite(name, full)
    for n in e.grads:
        got = cf.run(e, ops, need=[n])
        _same(f"{name}, {n} alone requires grad", got, (full[0], {n: full[1][n]}))
    with torch.no_grad():
        _same(f"{name} under no_grad", cf.run(e, ops, need=[]), (full[0], {}))
    with torch.inference_mode():
        _same(f"{name} under inference_mode", cf.run(e, ops, need=[]), (full[0], {}))


# ------------------------------------------------------------------------------------------------ 7. poincare_distance under grad
def test_poincare_distance_refuses_an_operand_that_requires_grad():
    from hypad_amd import _C
    from hypad_amd.hyperspace.poincare_distance import poincare_distance
    ops = _cuda(_entry("poincare_distance 39x65").build(8))
    pred, gt = ops["pred"], ops["gt"]
    plain = poincare_distance(pred, gt)
    assert plain.shape == (39, 65) and not plain.requires_grad
    for a, b in ((pred.clone().requires_grad_(True), gt), (pred, gt.clone().requires_grad_(True))):
        with pytest.raises(_C.HypadError, match=r"gmath\.dist_matmul"):
            poincare_distance(a, b)
        with torch.no_grad():
            assert torch.equal(poincare_distance(a, b), plain)
        assert torch.equal(poincare_distance(a.detach(), b.detach()), plain)
