"""The case table of tests/test_gpu_layer_call_forms.py and tests/test_layer_call_forms_host.py: one entry per first-generation layer
function -- the ones written before the wrappers began to refuse what they do not implement (hyperspace/gmath.py: expmap0, logmap0,
project, mobius_add, mobius_pointwise_mul, mobius_scalar_mul, mobius_fn_apply, mobius_matvec, dist2plane, poincare_rowdist,
hyperbolic_loss; hyperspace/hyrnn_nets.py; hyperspace/poincare_distance.py; hypad_amd/autograd.py) --, each as

    name, covers      the entry's name and the public names it stands for in the registry check ("gmath.expmap0", ...)
    build(seed, rows=None, small=False)
                      -> {operand name: float32 host tensor} in a fixed order, the grad_outputs (``gos``) among them.  rows=None: the
                      canonical shapes -- 39 rows; D = 100; 33 -> 17 for the layers; (17, 33, 63) for the GRU; T = 3 for the sequence
                      forms.  small=True: D = 5 for the row ops (the rank cases).  Ball rows come from sweep_common._ball_rows with
                      no rim row and no zero row.
    call(ops)         -> the tuple of outputs through the public function, from a dict of device tensors
    ref(ops)          -> the same call in plain torch in the dtype of its operands: oracle.gmath where it has the function,
                      tests/dist2plane_ref.py, tests/mobius_gru_ref.py, tests/midpoint_ref.py otherwise, torch's own
                      nn.functional.linear / nn.LSTM for autograd.*
    rows              {operand name: the axis that counts rows}; params: the parameters and one-row operands; both get gradients
    out_axes          per output, the axis that counts rows (None: the output has none -- hyperbolic_loss)
    ranks             "flat": the row operands take any number of leading dimensions; "refused": the function takes one fixed rank
                      and refuses another; None: the form has no meaning (the sequence forms)
    twice             the two operands that may be one tensor, or None
    dim_call(dim), k_call(k), k_none
                      the call on host tensors with 3-D row operands and that ``dim`` / ``k`` (None: the function takes none);
                      k_none: k=None is part of the signature

``run`` and ``reference`` are the two ways through an entry: the public function on device operands, and the plain-torch restatement on
the CPU.  The shapes are the smallest that still take the tail and a second row group: 39 rows are nine 4-row groups plus 3 and two
16-row tiles plus 7.
"""
from types import SimpleNamespace

import torch

import dist2plane_ref as d2r
import midpoint_ref as mr
import mobius_gru_ref as gr
from layers_on_streams_cases import LSTM_NAMES, ROWS, _ball, _gen, _lstm_params, _uniform
from oracle import gmath as og
from sweep_common import _ball_rows

D, D_SMALL = 100, 5
IN, OUT = 33, 17
GRU_ROWS, GRU_IN, GRU_HID = 17, 33, 63
T = 3
LSTM_H = 17


class Entry:
    def __init__(self, name, covers, build, call, ref, rows, params=(), gos=("go",), out_axes=(0,), ranks="flat", twice=None,
                 dim_call=None, k_call=None, k_none=False):
        self.name, self.covers, self.build, self.call, self.ref = name, tuple(covers), build, call, ref
        self.rows, self.params, self.gos, self.out_axes, self.ranks, self.twice = dict(rows), tuple(params), tuple(gos), tuple(out_axes), ranks, twice
        self.dim_call, self.k_call, self.k_none = dim_call, k_call, k_none
        self.grads = (tuple(self.rows) + self.params) if self.gos else ()

    def __repr__(self):
        return self.name

    def operands(self, ops):
        """The names of the tensors the call reads, in the order of ``build``."""
        return [n for n in ops if n not in self.gos]


def run(entry, ops, need=None, gos=None, shared=None):
    """([outputs], {operand name: gradient}) of the entry's public function on device operands.  The leaves are made over the operands
    themselves, so a view stays a view.  need: the operands that require grad (default: all of entry.grads); gos: the grad_outputs
    (default: the entry's own); shared: (a, b) -- both names get one and the same leaf."""
    need = entry.grads if need is None else tuple(need)
    leaves = {n: (ops[n].detach().requires_grad_(True) if n in need else ops[n].detach()) for n in entry.operands(ops)}
    if shared:
        leaves[shared[1]] = leaves[shared[0]]
        need = tuple(n for n in need if n != shared[1])
    outs = entry.call(leaves)
    if not need:
        return [o.detach() for o in outs], {}
    gs = torch.autograd.grad(outs, [leaves[n] for n in need], [ops[g] for g in entry.gos] if gos is None else gos)
    return [o.detach() for o in outs], dict(zip(need, gs))


def reference(entry, host, dtype):
    """The same through ``ref`` on the CPU in ``dtype``."""
    leaves = {n: host[n].detach().to(dtype).clone().requires_grad_(n in entry.grads) for n in entry.operands(host)}
    outs = entry.ref(leaves)
    if not entry.grads:
        return [o.detach() for o in outs], {}
    gs = torch.autograd.grad(outs, [leaves[n] for n in entry.grads], [host[g].to(dtype) for g in entry.gos])
    return [o.detach() for o in outs], dict(zip(entry.grads, gs))


def with_lead(entry, ops, lead):
    """The operands with the row axis of every row operand (and of every grad_output that has one) reshaped to ``lead``."""
    def shaped(t, axis):
        return t.reshape((*t.shape[:axis], *lead, *t.shape[axis + 1:]))
    out = dict(ops)
    for n, axis in entry.rows.items():
        out[n] = shaped(ops[n], axis)
    for g, axis in zip(entry.gos, entry.out_axes):
        if axis is not None:
            out[g] = shaped(ops[g], axis)
    return out


def _n(rows, default=ROWS):
    return default if rows is None else rows


def _tangent(g, rows, dim):
    return _ball_rows(g, rows, dim, tangent=True, zero_row=False)


Z = torch.zeros


# ------------------------------------------------------------------------------------------------ gmath
def _gmath_entries():
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace.poincare_distance import poincare_distance
    out = []

    def unary(name, fn, ref, tangent=False):
        def build(seed, rows=None, small=False):
            g, d = _gen(seed), D_SMALL if small else D
            x = _tangent(g, _n(rows), d) if tangent else _ball(g, _n(rows), d)
            return dict(x=x, go=torch.randn(_n(rows), d, generator=g))
        return Entry("gmath." + name, ["gmath." + name], build, lambda o: (fn(o["x"]),), lambda o: (ref(o["x"]),), rows=dict(x=0),
                     dim_call=lambda dim: fn(Z(2, 3, 8), dim=dim), k_call=lambda k: fn(Z(2, 3, 8), k=k), k_none=True)
    fn_apply = lambda x, **kw: gmath.mobius_fn_apply(torch.tanh, x, **kw)
    out += [unary("expmap0", gmath.expmap0, og.expmap0, tangent=True), unary("logmap0", gmath.logmap0, og.logmap0),
            unary("project", gmath.project, og.project),
            unary("mobius_fn_apply", fn_apply, lambda x: og.expmap0(torch.tanh(og.logmap0(x))))]

    def binary(name, fn, ref, first, second, one_row):
        """fn(a, b) with a = ops[first] of all rows and b = ops[second] of all rows or of one."""
        def build(seed, rows=None, small=False):
            g, d = _gen(seed), D_SMALL if small else D
            a, b = _ball(g, _n(rows), d), _ball(g, 1 if one_row else _n(rows), d, radius=0.5)
            return {first: a, second: b[0] if one_row else b, "go": torch.randn(_n(rows), d, generator=g)}
        host = lambda: (Z(2, 3, 8), Z(8) if one_row else Z(2, 3, 8))
        return Entry(f"gmath.{name}" + (f", {second} of one row" if one_row else ""), ["gmath." + name], build,
                     lambda o: (fn(o[first], o[second]),), lambda o: (ref(o[first], o[second]),),
                     rows={first: 0} if one_row else {first: 0, second: 0}, params=(second,) if one_row else (),
                     twice=None if one_row else (first, second), dim_call=lambda dim: fn(*host(), dim=dim), k_call=lambda k: fn(*host(), k=k),
                     k_none=True)
    pmul = lambda x, w, **kw: gmath.mobius_pointwise_mul(w, x, **kw)
    pmul_ref = lambda x, w: gr.pointwise_mul_ref(w, x)
    out += [binary("mobius_add", gmath.mobius_add, og.mobius_add, "x", "y", False),
            binary("mobius_add", gmath.mobius_add, og.mobius_add, "x", "y", True),
            binary("mobius_pointwise_mul", pmul, pmul_ref, "x", "w", False), binary("mobius_pointwise_mul", pmul, pmul_ref, "x", "w", True)]

    def smul(per_row):
        def build(seed, rows=None, small=False):
            g, d = _gen(seed), D_SMALL if small else D
            r = _uniform(g, _n(rows), 1, bound=1.5) if per_row else _uniform(g, 1, bound=1.5)
            return dict(r=r, x=_ball(g, _n(rows), d), go=torch.randn(_n(rows), d, generator=g))
        host = lambda: (Z(2, 3, 1) if per_row else Z(1), Z(2, 3, 8))
        return Entry("gmath.mobius_scalar_mul, " + ("r per row" if per_row else "r of one element"), ["gmath.mobius_scalar_mul"], build,
                     lambda o: (gmath.mobius_scalar_mul(o["r"], o["x"]),), lambda o: (mr.mobius_scalar_mul_ref(o["r"], o["x"]),),
                     rows=dict(r=0, x=0) if per_row else dict(x=0), params=() if per_row else ("r",),
                     dim_call=lambda dim: gmath.mobius_scalar_mul(*host(), dim=dim), k_call=lambda k: gmath.mobius_scalar_mul(*host(), k=k),
                     k_none=True)
    out += [smul(False), smul(True)]

    def matvec_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(m=_uniform(g, OUT, IN, bound=IN ** -0.5), x=_ball(g, _n(rows), IN), go=torch.randn(_n(rows), OUT, generator=g))
    out.append(Entry("gmath.mobius_matvec 33->17", ["gmath.mobius_matvec"], matvec_build, lambda o: (gmath.mobius_matvec(o["m"], o["x"]),),
                     lambda o: (gr.matvec_scaled(o["x"] @ o["m"].t(), o["x"]),), rows=dict(x=0), params=("m",),
                     dim_call=lambda dim: gmath.mobius_matvec(Z(5, 8), Z(2, 3, 8), dim=dim),
                     k_call=lambda k: gmath.mobius_matvec(Z(5, 8), Z(2, 3, 8), k=k), k_none=True))

    def d2p_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(x=_ball(g, _n(rows), IN).reshape(_n(rows), 1, IN), p=_ball(g, OUT, IN, radius=0.7), a=torch.randn(OUT, IN, generator=g),
                    go=torch.randn(_n(rows), OUT, generator=g))
    d2p = lambda x, p, a, **kw: gmath.dist2plane(x, p, a, signed=True, scaled=True, **kw)
    out.append(Entry("gmath.dist2plane(signed, scaled) 33->17", ["gmath.dist2plane"], d2p_build, lambda o: (d2p(o["x"], o["p"], o["a"]),),
                     lambda o: (d2r.dist2plane_ref(o["x"].squeeze(-2), o["p"], o["a"], signed=True, scaled=True),), rows=dict(x=0),
                     params=("p", "a"), dim_call=lambda dim: d2p(Z(2, 1, 8), Z(5, 8), Z(5, 8), dim=dim),
                     k_call=lambda k: d2p(Z(2, 1, 8), Z(5, 8), Z(5, 8), k=k), k_none=True))

    def uv_build(go):
        def build(seed, rows=None, small=False):
            g, d = _gen(seed), D_SMALL if small else D
            return dict(u=_ball(g, _n(rows), d), v=_ball(g, _n(rows), d), go=go(g, _n(rows)))
        return build
    out.append(Entry("gmath.poincare_rowdist", ["gmath.poincare_rowdist"], uv_build(lambda g, rows: torch.randn(rows, generator=g)),
                     lambda o: (gmath.poincare_rowdist(o["u"], o["v"]),), lambda o: (og.rowwise_poincare_distance(o["u"], o["v"]),),
                     rows=dict(u=0, v=0), twice=("u", "v")))
    # (the incoming gradient is a scalar that is not 1; the batch size does not divide it exactly)
    out.append(Entry("gmath.hyperbolic_loss", ["gmath.hyperbolic_loss"], uv_build(lambda g, rows: torch.rand((), generator=g) + 0.25),
                     lambda o: (gmath.hyperbolic_loss(o["u"], o["v"], ROWS),),
                     lambda o: (og.rowwise_poincare_distance(o["u"], o["v"]).sum() / ROWS,), rows=dict(u=0, v=0), out_axes=(None,),
                     twice=("u", "v")))

    def pair_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(pred=_ball(g, _n(rows), IN), gt=_ball(g, 65, IN))

    def pair_call(o):
        with torch.no_grad():
            return (poincare_distance(o["pred"], o["gt"]),)
    out.append(Entry("poincare_distance 39x65", ["poincare_distance.poincare_distance"], pair_build, pair_call,
                     lambda o: (og.pairwise_poincare_distance(o["pred"], o["gt"]),), rows=dict(pred=0), gos=(), ranks="refused",
                     twice=("pred", "gt")))
    return out


# ------------------------------------------------------------------------------------------------ hyrnn_nets
def _set(module, **tensors):
    """The module with the named parameters replaced by the given tensors themselves (leaves of the caller's graph)."""
    for n, t in tensors.items():
        del module._parameters[n]
        setattr(module, n, t)
    return module


def _mobius_linear_ref(x, w, b, hyper_in, nonlin=None):
    """hyperspace/hyrnn_nets.py:13-35 with a ball-valued bias."""
    out = gr.matvec_scaled(x @ w.t(), x) if hyper_in else og.expmap0(x @ w.t())
    out = og.mobius_add(out, b.expand_as(out))
    if nonlin is not None:
        out = og.expmap0(nonlin(og.logmap0(out)))
    return og.project(out)


def _hyrnn_entries():
    from hypad_amd.hyperspace import hyrnn_nets as hn
    out = []

    def linear_build(hyper_in):
        def build(seed, rows=None, small=False):
            g = _gen(seed)
            x = _ball(g, _n(rows), IN) if hyper_in else torch.randn(_n(rows), IN, generator=g)
            return dict(x=x, weight=_uniform(g, OUT, IN, bound=IN ** -0.5), bias=_ball(g, 1, OUT, radius=0.5)[0],
                        go=torch.randn(_n(rows), OUT, generator=g))
        return build

    def linear(hyper_in, nonlin, tag):
        fn = lambda x, w, b, **kw: hn.mobius_linear(x, w, b, hyperbolic_input=hyper_in, hyperbolic_bias=True, nonlin=nonlin, **kw)
        return Entry(f"hyrnn_nets.mobius_linear 33->17, {tag}", ["hyrnn_nets.mobius_linear"], linear_build(hyper_in),
                     lambda o: (fn(o["x"], o["weight"], o["bias"]),),
                     lambda o: (_mobius_linear_ref(o["x"], o["weight"], o["bias"], hyper_in, nonlin),), rows=dict(x=0),
                     params=("weight", "bias"), k_call=lambda k: fn(Z(2, 3, 8), Z(5, 8), Z(5), k=k))
    out += [linear(False, None, "Euclidean input, ball bias"), linear(True, torch.tanh, "ball input, ball bias, tanh")]

    def matvec_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(m=_uniform(g, OUT, IN, bound=IN ** -0.5), x=_ball(g, _n(rows), IN), go=torch.randn(_n(rows), OUT, generator=g))
    out.append(Entry("hyrnn_nets.mobius_matvec 33->17", ["hyrnn_nets.mobius_matvec"], matvec_build,
                     lambda o: (hn.mobius_matvec(o["m"], o["x"], k=-1.0),), lambda o: (gr.matvec_scaled(o["x"] @ o["m"].t(), o["x"]),),
                     rows=dict(x=0), params=("m",), dim_call=lambda dim: hn.mobius_matvec(Z(5, 8), Z(2, 3, 8), k=-1.0, dim=dim),
                     k_call=lambda k: hn.mobius_matvec(Z(5, 8), Z(2, 3, 8), k=k)))

    def rnn_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(W=_uniform(g, OUT, IN, bound=IN ** -0.5), h=_ball(g, _n(rows), IN), U=_uniform(g, OUT, IN, bound=IN ** -0.5),
                    x=_ball(g, _n(rows), IN), b=_ball(g, 1, OUT, radius=0.5)[0], go=torch.randn(_n(rows), OUT, generator=g))
    out.append(Entry("hyrnn_nets.one_rnn_transform 33->17", ["hyrnn_nets.one_rnn_transform"], rnn_build,
                     lambda o: (hn.one_rnn_transform(o["W"], o["h"], o["U"], o["x"], o["b"], -1.0),),
                     lambda o: (gr.transform(o["h"] @ o["W"].t(), o["h"], o["x"] @ o["U"].t(), o["x"], o["b"]),), rows=dict(h=0, x=0),
                     params=("W", "U", "b"), twice=("h", "x"),
                     k_call=lambda k: hn.one_rnn_transform(Z(5, 8), Z(2, 3, 8), Z(5, 8), Z(2, 3, 8), Z(5), k)))

    def gru_build(steps):
        def build(seed, rows=None, small=False):
            g, n = _gen(seed), _n(rows, GRU_ROWS)
            x = _ball(g, (steps or 1) * n, GRU_IN)
            lead = (n,) if steps is None else (steps, n)
            d = dict(x=x.reshape(*lead, GRU_IN), h0=_ball(g, n, GRU_HID), weight_ih=_uniform(g, 3 * GRU_HID, GRU_IN, bound=GRU_HID ** -0.5),
                     weight_hh=_uniform(g, 3 * GRU_HID, GRU_HID, bound=GRU_HID ** -0.5), bias=_ball(g, 3, GRU_HID, radius=0.5),
                     go=torch.randn(*lead, GRU_HID, generator=g))
            if steps is not None:
                d["go_last"] = torch.randn(n, GRU_HID, generator=g)
            return d
        return build
    names = ("x", "h0", "weight_ih", "weight_hh", "bias")
    host = lambda *lead: (Z(*lead, 3, 8), Z(3, 4), Z(12, 8), Z(12, 4), Z(3, 4))
    out.append(Entry("hyrnn_nets.mobius_gru_cell (17, 33, 63)", ["hyrnn_nets.mobius_gru_cell"], gru_build(None),
                     lambda o: (hn.mobius_gru_cell(*(o[n] for n in names), -1.0),), lambda o: (gr.gru_cell_ref(*(o[n] for n in names)),),
                     rows=dict(x=0, h0=0), params=names[2:], ranks="refused", k_call=lambda k: hn.mobius_gru_cell(*host(), k)))

    def loop(o):
        return hn.mobius_gru_loop(*(o[n] for n in names), -1.0, hyperbolic_input=True, hyperbolic_hidden_state0=True)
    out.append(Entry("hyrnn_nets.mobius_gru_loop T = 3 (17, 33, 63)", ["hyrnn_nets.mobius_gru_loop"], gru_build(T), loop,
                     lambda o: gr.gru_loop_ref(*(o[n] for n in names))[:2], rows=dict(x=1, h0=0), params=names[2:], gos=("go", "go_last"),
                     out_axes=(1, 0), ranks=None, k_call=lambda k: hn.mobius_gru_loop(*host(2), k)))

    def layer_call(o):
        layer = _set(hn.MobiusLinear(IN, OUT, fp64_hyper=False), weight=o["weight"], bias=o["bias"])
        return (layer(o["x"]),)
    out.append(Entry("hyrnn_nets.MobiusLinear(33, 17) on the ball", ["hyrnn_nets.MobiusLinear"], linear_build(True), layer_call,
                     lambda o: (_mobius_linear_ref(o["x"], o["weight"], o["bias"], True),), rows=dict(x=0), params=("weight", "bias"),
                     k_call=lambda k: hn.MobiusLinear(8, 5, fp64_hyper=False, k=k)(Z(2, 3, 8))))

    def d2p_build(seed, rows=None, small=False):
        g = _gen(seed)
        a = torch.randn(OUT, IN, generator=g)
        return dict(x=_ball(g, _n(rows), IN), point=_ball(g, OUT, IN, radius=0.7), tangent=a / a.norm(dim=1, keepdim=True),
                    scale=_uniform(g, OUT, bound=0.5), go=torch.randn(_n(rows), OUT, generator=g))

    def d2p_call(o):
        layer = _set(hn.MobiusDist2Hyperplane(IN, OUT), point=o["point"], tangent=o["tangent"], scale=o["scale"])
        return (layer(o["x"]),)
    out.append(Entry("hyrnn_nets.MobiusDist2Hyperplane(33, 17)", ["hyrnn_nets.MobiusDist2Hyperplane"], d2p_build, d2p_call,
                     lambda o: (d2r.layer_ref(o["x"], o["point"], o["tangent"], o["scale"]),), rows=dict(x=0),
                     params=("point", "tangent", "scale"), k_call=lambda k: hn.MobiusDist2Hyperplane(8, 5, k=k)(Z(2, 3, 8))))
    return out


# ------------------------------------------------------------------------------------------------ autograd
def _torch_lstm(o):
    """torch's own nn.LSTM over the operands' eight tensors (leaves of the caller's graph), in their dtype."""
    lstm = torch.nn.LSTM(o[LSTM_NAMES[0]].shape[1], o[LSTM_NAMES[1]].shape[1], bidirectional=True)
    return _set(lstm, **{n: o[n] for n in LSTM_NAMES})


def _autograd_entries():
    from hypad_amd import _C, autograd as hag
    out = []

    def lin_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(x=torch.randn(_n(rows), IN, generator=g), weight=_uniform(g, OUT, IN, bound=IN ** -0.5), bias=_uniform(g, OUT, bound=0.3),
                    go=torch.randn(_n(rows), OUT, generator=g))
    out.append(Entry("autograd.linear_act 33->17, tanh", ["autograd.linear_act"], lin_build,
                     lambda o: (hag.linear_act(o["x"], o["weight"], o["bias"], _C.ACT_TANH),),
                     lambda o: (torch.tanh(torch.nn.functional.linear(o["x"], o["weight"], o["bias"])),), rows=dict(x=0),
                     params=("weight", "bias"), ranks="refused"))

    def holder(o):
        return SimpleNamespace(parameters=lambda: iter([o[n] for n in LSTM_NAMES]), **{n: o[n] for n in LSTM_NAMES})

    def layer_build(seed, rows=None, small=False):
        g = _gen(seed)
        return dict(x=torch.randn(_n(rows), IN, generator=g), **_lstm_params(g, IN, LSTM_H), go=torch.randn(_n(rows), 2 * LSTM_H, generator=g))
    out.append(Entry("autograd.lstm_layer 33->2x17", ["autograd.lstm_layer"], layer_build, lambda o: (hag.lstm_layer(o["x"], holder(o), 0),),
                     lambda o: (_torch_lstm(o)(o["x"].unsqueeze(0))[0][0],), rows=dict(x=0), params=LSTM_NAMES, ranks="refused"))

    def seq_build(grads):
        def build(seed, rows=None, small=False):
            g, n = _gen(seed), _n(rows)
            d = dict(x=torch.randn(T, n, IN, generator=g), h0=0.5 * torch.randn(2, n, LSTM_H, generator=g),
                     c0=0.5 * torch.randn(2, n, LSTM_H, generator=g), **_lstm_params(g, IN, LSTM_H))
            if grads:
                d.update(go_out=torch.randn(T, n, 2 * LSTM_H, generator=g), go_hn=torch.randn(2, n, LSTM_H, generator=g),
                         go_cn=torch.randn(2, n, LSTM_H, generator=g))
            return d
        return build

    def seq_ref(o):
        res, (hn, cn) = _torch_lstm(o)(o["x"], (o["h0"], o["c0"]))
        return res, hn, cn

    def seq_call(o):
        res, (hn, cn) = hag.lstm_seq(o["x"], holder(o), 0, (o["h0"], o["c0"]))
        return res, hn, cn

    def fwd_call(o):
        with torch.no_grad():
            res, (hn, cn) = hag.lstm_seq_forward(o["x"], holder(o), 0, (o["h0"], o["c0"]))
        return res, hn, cn
    seq_rows = dict(x=1, h0=1, c0=1)
    out.append(Entry("autograd.lstm_seq T = 3, 33->2x17, with h0 and c0", ["autograd.lstm_seq"], seq_build(True), seq_call, seq_ref, rows=seq_rows,
                     params=LSTM_NAMES, gos=("go_out", "go_hn", "go_cn"), out_axes=(1, 1, 1), ranks=None))
    out.append(Entry("autograd.lstm_seq_forward T = 3, 33->2x17, with h0 and c0", ["autograd.lstm_seq_forward"], seq_build(False), fwd_call,
                     seq_ref, rows=seq_rows, gos=(), out_axes=(1, 1, 1), ranks=None))
    return out


def entries():
    return _gmath_entries() + _hyrnn_entries() + _autograd_entries()


# (the names alone, for parametrisation at collection time without importing the package)
NAMES = [
    "gmath.expmap0", "gmath.logmap0", "gmath.project", "gmath.mobius_fn_apply", "gmath.mobius_add", "gmath.mobius_add, y of one row",
    "gmath.mobius_pointwise_mul", "gmath.mobius_pointwise_mul, w of one row", "gmath.mobius_scalar_mul, r of one element",
    "gmath.mobius_scalar_mul, r per row", "gmath.mobius_matvec 33->17", "gmath.dist2plane(signed, scaled) 33->17", "gmath.poincare_rowdist",
    "gmath.hyperbolic_loss", "poincare_distance 39x65", "hyrnn_nets.mobius_linear 33->17, Euclidean input, ball bias",
    "hyrnn_nets.mobius_linear 33->17, ball input, ball bias, tanh", "hyrnn_nets.mobius_matvec 33->17", "hyrnn_nets.one_rnn_transform 33->17",
    "hyrnn_nets.mobius_gru_cell (17, 33, 63)", "hyrnn_nets.mobius_gru_loop T = 3 (17, 33, 63)", "hyrnn_nets.MobiusLinear(33, 17) on the ball",
    "hyrnn_nets.MobiusDist2Hyperplane(33, 17)", "autograd.linear_act 33->17, tanh", "autograd.lstm_layer 33->2x17",
    "autograd.lstm_seq T = 3, 33->2x17, with h0 and c0", "autograd.lstm_seq_forward T = 3, 33->2x17, with h0 and c0"]
WITH_GRADS = [n for n in NAMES if not n.startswith(("poincare_distance", "autograd.lstm_seq_forward"))]
FLAT = [n for n in WITH_GRADS if not n.startswith(("hyrnn_nets.mobius_gru", "autograd."))]
REFUSED_RANKS = ["poincare_distance 39x65", "hyrnn_nets.mobius_gru_cell (17, 33, 63)", "autograd.linear_act 33->17, tanh",
                 "autograd.lstm_layer 33->2x17"]
TWICE = ["gmath.mobius_add", "gmath.mobius_pointwise_mul", "gmath.poincare_rowdist", "gmath.hyperbolic_loss", "poincare_distance 39x65",
         "hyrnn_nets.one_rnn_transform 33->17"]
WITH_DIM = ["gmath.expmap0", "gmath.logmap0", "gmath.project", "gmath.mobius_fn_apply", "gmath.mobius_add", "gmath.mobius_add, y of one row",
            "gmath.mobius_pointwise_mul", "gmath.mobius_pointwise_mul, w of one row", "gmath.mobius_scalar_mul, r of one element",
            "gmath.mobius_scalar_mul, r per row", "gmath.mobius_matvec 33->17", "gmath.dist2plane(signed, scaled) 33->17",
            "hyrnn_nets.mobius_matvec 33->17"]
WITH_K = WITH_DIM[:-1] + ["hyrnn_nets.mobius_linear 33->17, Euclidean input, ball bias", "hyrnn_nets.mobius_linear 33->17, ball input, ball bias, tanh",
                     "hyrnn_nets.mobius_matvec 33->17", "hyrnn_nets.one_rnn_transform 33->17", "hyrnn_nets.mobius_gru_cell (17, 33, 63)",
                     "hyrnn_nets.mobius_gru_loop T = 3 (17, 33, 63)", "hyrnn_nets.MobiusLinear(33, 17) on the ball",
                     "hyrnn_nets.MobiusDist2Hyperplane(33, 17)"]

# Every other public function and module of the four files, with the test that holds its own calling forms.
_NEWER = "tests/test_gpu_{}.py::test_refusals_write_nothing"
COVERED_ELSEWHERE = {
    **{f"gmath.{n}": _NEWER.format("weighted_midpoint") for n in ("weighted_midpoint", "weighted_midpoint_bmm")},
    **{f"gmath.{n}": _NEWER.format("dist") for n in ("dist_matmul", "dist", "dist0")},
    "gmath.hyperbolic_attention": _NEWER.format("attention"),
    "gmath.dist2plane_matmul": _NEWER.format("dist2plane_matmul"),
    **{f"gmath.{n}": _NEWER.format("tangent_maps") for n in ("expmap", "logmap", "geodesic", "gyration", "parallel_transport", "parallel_transport0",
                                                            "parallel_transport0back")},
    **{f"gmath.{n}": _NEWER.format("gyro_ops") for n in ("mobius_sub", "mobius_coadd", "mobius_cosub", "geodesic_unit", "lambda_x", "inner", "norm",
                                                        "egrad2rgrad", "sproj", "inv_sproj")},
    **{f"gmath.{n}": "tests/test_gyro_ops_host.py::test_functions_without_a_kernel" for n in ("antipode", "mobius_fn_apply_chain", "mobiusify")},
    **{f"autograd.{n}": "tests/test_gpu_autograd_r2.py::test_module_forwards_are_differentiable"
       for n in ("wants_graph", "encoder_forward", "decoder_forward", "critic_forward")},
}
