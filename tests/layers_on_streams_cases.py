"""The case table of tests/test_gpu_layers_on_streams.py: every differentiable layer a caller reaches "outside the fused iterations"
(hypad_amd/autograd.py, hyperspace/gmath.py, hyperspace/hyrnn_nets.py, hyperspace/poincare_distance.py, hypad_amd/optim.py), each as

    name
    build(seed)  -> {operand name: float32 host tensor}, in a fixed order; ball-valued data from sweep_common._ball_rows
    place(host)  -> {operand name: uninitialised device buffer of that shape} plus, under keys that start with "_", whatever object the
                    call needs around the buffers (a module whose parameters ARE the buffers)
    run(ops)     -> [outputs..., gradients...] through the public Python functions: the forward, then torch.autograd.grad with a fixed
                    grad_outputs operand that is itself one of the case's buffers
    graph        -> False for the optimisers (they take the step number by value: hypad_amd/optim.py)

Nothing here compares numbers with a reference: the two tests hold a run on a side stream, and a captured run replayed queued, to the
bits of an eager run of the same code on the default stream, whose numbers the sweeps hold to fp64.  The shapes are the smallest that
still take the multi-launch and tail paths: 39 rows (nine 4-row groups plus 3; two 16-row tiles plus 7) unless the name says otherwise.
The data stays clear of what produces a NaN (no rim row, no zero row): a NaN in an expected tensor would compare unequal to itself.
"""
from types import SimpleNamespace

import torch

from sweep_common import _ball_rows

ROWS = 39
LSTM_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0",
              "weight_ih_l0_reverse", "weight_hh_l0_reverse", "bias_ih_l0_reverse", "bias_hh_l0_reverse")


class Case:
    def __init__(self, name, build, run, place=None, graph=True):
        self.name, self.build, self.run, self.graph = name, build, run, graph
        self.place = place or _place

    def __repr__(self):
        return self.name


def _place(host):
    return {k: torch.empty(v.shape, dtype=v.dtype, device="cuda") for k, v in host.items()}


def _gen(seed):
    return torch.Generator().manual_seed(7919 * seed + 13)


def _ball(g, rows, dim, radius=0.9):
    return _ball_rows(g, rows, dim, zero_row=False, edge=False, radius=radius)


def _leaf(t):
    """A fresh leaf over the buffer itself (no copy: the run reads what the buffer holds when its kernels execute)."""
    return t.detach().requires_grad_(True)


def _fwd_bwd(fn, ops, names, go="go"):
    """[out, gradients of the named operands under ops[go]]."""
    leaves = [_leaf(ops[n]) for n in names]
    out = fn(*leaves)
    return [out.detach(), *torch.autograd.grad(out, leaves, ops[go])]


def _uniform(g, *shape, bound=1.0):
    return (torch.rand(*shape, generator=g) * 2 - 1) * bound


# ------------------------------------------------------------------------------------------------ gmath
def _gmath_cases():
    from hypad_amd.hyperspace import gmath, poincare_distance as pd
    D = 100
    out = []

    def unary(name, fn, tangent):
        def build(seed):
            g = _gen(seed)
            x = _ball_rows(g, ROWS, D, tangent=True, zero_row=False) if tangent else _ball(g, ROWS, D)
            return dict(x=x, go=torch.randn(ROWS, D, generator=g))
        return Case(name, build, lambda ops: _fwd_bwd(fn, ops, ["x"]))
    out += [unary("gmath.expmap0", gmath.expmap0, True), unary("gmath.logmap0", gmath.logmap0, False),
            unary("gmath.project", gmath.project, False),
            unary("gmath.mobius_fn_apply(tanh)", lambda x: gmath.mobius_fn_apply(torch.tanh, x), False)]

    def binary(name, fn, one_row, first="x", second="y"):
        def build(seed):
            g = _gen(seed)
            a, b = _ball(g, ROWS, D), _ball(g, 1 if one_row else ROWS, D, radius=0.5)
            return {first: a, second: b[0] if one_row else b, "go": torch.randn(ROWS, D, generator=g)}
        return Case(name, build, lambda ops: _fwd_bwd(fn, ops, [first, second]))
    pmul = lambda x, w: gmath.mobius_pointwise_mul(w, x)
    out += [binary("gmath.mobius_add", gmath.mobius_add, False), binary("gmath.mobius_add, y of one row", gmath.mobius_add, True),
            binary("gmath.mobius_pointwise_mul", pmul, False, "x", "w"),
            binary("gmath.mobius_pointwise_mul, w of one row", pmul, True, "x", "w")]

    def uv(seed, go):
        g = _gen(seed)
        return dict(u=_ball(g, ROWS, D), v=_ball(g, ROWS, D), go=go(g))
    out.append(Case("gmath.poincare_rowdist", lambda seed: uv(seed, lambda g: torch.randn(ROWS, generator=g)),
                    lambda ops: _fwd_bwd(gmath.poincare_rowdist, ops, ["u", "v"])))
    # the incoming gradient is a device scalar that is not 1; the batch size does not divide it exactly
    out.append(Case("gmath.hyperbolic_loss", lambda seed: uv(seed, lambda g: torch.rand((), generator=g) + 0.25),
                    lambda ops: _fwd_bwd(lambda u, v: gmath.hyperbolic_loss(u, v, ROWS), ops, ["u", "v"])))

    def matvec(seed):
        g = _gen(seed)
        return dict(m=_uniform(g, 63, 33, bound=33 ** -0.5), x=_ball(g, ROWS, 33), go=torch.randn(ROWS, 63, generator=g))
    out.append(Case("gmath.mobius_matvec 33->63", matvec, lambda ops: _fwd_bwd(gmath.mobius_matvec, ops, ["m", "x"])))

    def d2p(seed):
        g = _gen(seed)
        return dict(x=_ball(g, ROWS, 33).reshape(ROWS, 1, 33), p=_ball(g, 17, 33, radius=0.7), a=torch.randn(17, 33, generator=g),
                    go=torch.randn(ROWS, 17, generator=g))
    out.append(Case("gmath.dist2plane(signed, scaled)", d2p,
                    lambda ops: _fwd_bwd(lambda x, p, a: gmath.dist2plane(x, p, a, signed=True, scaled=True), ops, ["x", "p", "a"])))

    def pair(seed):
        g = _gen(seed)
        return dict(pred=_ball(g, 65, 33), gt=_ball(g, 130, 33))
    out.append(Case("poincare_distance 65x130", pair, lambda ops: [pd.poincare_distance(ops["pred"], ops["gt"])]))
    return out


# ------------------------------------------------------------------------------------------------ hyrnn_nets
def _hyrnn_cases():
    from hypad_amd.hyperspace import hyrnn_nets as hn
    out = []

    def linear(hyper_in, hyper_bias, nonlin):
        def build(seed):
            g = _gen(seed)
            x = _ball(g, ROWS, 33) if hyper_in else torch.randn(ROWS, 33, generator=g)
            b = _ball(g, 1, 63, radius=0.5)[0] if hyper_bias else _uniform(g, 63, bound=0.3)
            return dict(x=x, weight=_uniform(g, 63, 33, bound=33 ** -0.5), bias=b, go=torch.randn(ROWS, 63, generator=g))
        fn = lambda x, w, b: hn.mobius_linear(x, w, b, hyperbolic_input=hyper_in, hyperbolic_bias=hyper_bias, nonlin=nonlin)
        name = (f"mobius_linear 33->63, {'ball' if hyper_in else 'Euclidean'} input, {'ball' if hyper_bias else 'Euclidean'} bias"
                + (", tanh" if nonlin is not None else ""))
        return Case(name, build, lambda ops: _fwd_bwd(fn, ops, ["x", "weight", "bias"]))
    out += [linear(False, True, None),                      # the original _MobiusLinearFn configuration
            linear(True, True, torch.tanh), linear(True, False, None), linear(False, False, None)]

    def d2p_build(seed):
        g = _gen(seed)
        a = torch.randn(17, 33, generator=g)
        return dict(x=_ball(g, ROWS, 33), point=_ball(g, 17, 33, radius=0.7), tangent=a / a.norm(dim=1, keepdim=True),
                    scale=_uniform(g, 17, bound=0.5), go=torch.randn(ROWS, 17, generator=g))

    def d2p_place(host):
        ops = _place(host)
        layer = hn.MobiusDist2Hyperplane(33, 17)
        for n in ("point", "tangent", "scale"):
            getattr(layer, n).data = ops[n]
        ops["_layer"] = layer
        return ops

    def d2p_run(ops):
        layer, x = ops["_layer"], _leaf(ops["x"])
        out_ = layer(x)
        return [out_.detach(), *torch.autograd.grad(out_, [x, layer.point, layer.tangent, layer.scale], ops["go"])]
    out.append(Case("MobiusDist2Hyperplane(33, 17)", d2p_build, d2p_run, d2p_place))

    def gru_build(rows, in_dim, hid, steps=None, packed=None, ball=True):
        def build(seed):
            g = _gen(seed)
            n = rows if steps is None else steps * rows
            n = sum(packed) if packed else n
            x = _ball(g, n, in_dim) if ball else 0.5 * torch.randn(n, in_dim, generator=g)
            h0 = _ball(g, rows, hid) if ball else 0.5 * torch.randn(rows, hid, generator=g)
            d = dict(x=x if steps is None else x.reshape(steps, rows, in_dim), h0=h0,
                     weight_ih=_uniform(g, 3 * hid, in_dim, bound=hid ** -0.5), weight_hh=_uniform(g, 3 * hid, hid, bound=hid ** -0.5),
                     bias=_ball(g, 3, hid, radius=0.5), go=torch.randn(*((n, hid) if steps is None else (steps, rows, hid)), generator=g))
            if packed:
                d["go_last"] = torch.randn(rows, hid, generator=g)
            return d
        return build
    GRU = ["x", "h0", "weight_ih", "weight_hh", "bias"]
    out.append(Case("mobius_gru_cell (17, 33, 63)", gru_build(17, 33, 63), lambda ops: _fwd_bwd(lambda *a: hn.mobius_gru_cell(*a, -1.0), ops, GRU)))

    def loop_run(ops):
        leaves = [_leaf(ops[n]) for n in GRU]
        outs, last = hn.mobius_gru_loop(*leaves, -1.0)
        return [outs.detach(), last.detach(), *torch.autograd.grad(outs, leaves, ops["go"])]
    out.append(Case("mobius_gru_loop T = 3 (17, 33, 63)", gru_build(17, 33, 63, steps=3, ball=False), loop_run))
    SIZES = [9, 7, 7, 4]

    def packed_run(ops):
        leaves = [_leaf(ops[n]) for n in GRU]
        outs, last = hn.mobius_gru_loop(*leaves, -1.0, batch_sizes=SIZES, hyperbolic_input=True, hyperbolic_hidden_state0=True)
        return [outs.detach(), last.detach(), *torch.autograd.grad([outs, last], leaves, [ops["go"], ops["go_last"]])]
    out.append(Case("mobius_gru_loop batch_sizes [9, 7, 7, 4]", gru_build(9, 33, 63, packed=SIZES), packed_run))
    return out


# ------------------------------------------------------------------------------------------------ autograd
def _lstm_params(g, K, H):
    shapes = [(4 * H, K), (4 * H, H), (4 * H,), (4 * H,)] * 2
    return {n: _uniform(g, *s, bound=H ** -0.5) for n, s in zip(LSTM_NAMES, shapes)}


def _autograd_cases():
    from hypad_amd import _C, autograd as hag
    out = []

    def lin_build(seed):
        g = _gen(seed)
        return dict(x=torch.randn(ROWS, 33, generator=g), weight=_uniform(g, 17, 33, bound=33 ** -0.5), bias=_uniform(g, 17, bound=0.3),
                    go=torch.randn(ROWS, 17, generator=g))
    for tag, act in (("none", _C.ACT_NONE), ("tanh", _C.ACT_TANH), ("leaky", _C.ACT_LEAKY02)):
        out.append(Case(f"autograd.linear_act 33->17, {tag}", lin_build,
                        lambda ops, act=act: _fwd_bwd(lambda x, w, b: hag.linear_act(x, w, b, act), ops, ["x", "weight", "bias"])))

    def layer_case(name, K, H, rows):
        def build(seed):
            g = _gen(seed)
            return dict(x=torch.randn(rows, K, generator=g), **_lstm_params(g, K, H), go=torch.randn(rows, 2 * H, generator=g))

        def run(ops):
            leaves = [_leaf(ops[n]) for n in ("x",) + LSTM_NAMES]
            out_ = hag.lstm_layer(leaves[0], SimpleNamespace(**dict(zip(LSTM_NAMES, leaves[1:]))), 0)
            return [out_.detach(), *torch.autograd.grad(out_, leaves, ops["go"])]
        return Case(name, build, run)
    out += [layer_case("autograd.lstm_layer 20->2x32, 39 rows (streamed)", 20, 32, ROWS),
            layer_case("autograd.lstm_layer 100->2x50, 2053 rows (weights-stationary, saved gates)", 100, 50, 2053)]

    T, R, K, H = 3, 21, 9, 33

    def seq_build(seed):
        g = _gen(seed)
        return dict(x=torch.randn(T, R, K, generator=g), h0=0.5 * torch.randn(2, R, H, generator=g), c0=0.5 * torch.randn(2, R, H, generator=g),
                    **_lstm_params(g, K, H), go_out=torch.randn(T, R, 2 * H, generator=g), go_hn=torch.randn(2, R, H, generator=g),
                    go_cn=torch.randn(2, R, H, generator=g))

    def seq_run(ops):
        leaves = [_leaf(ops[n]) for n in ("x", "h0", "c0") + LSTM_NAMES]
        o, (hn_, cn) = hag.lstm_seq(leaves[0], SimpleNamespace(**dict(zip(LSTM_NAMES, leaves[3:]))), 0, (leaves[1], leaves[2]))
        return [o.detach(), hn_.detach(), cn.detach(),
                *torch.autograd.grad([o, hn_, cn], leaves, [ops["go_out"], ops["go_hn"], ops["go_cn"]])]
    out.append(Case("autograd.lstm_seq T = 3, 21 rows, 9->2x33, with h0 and c0", seq_build, seq_run))
    return out


def _module_cases():
    """The models.tadgan modules at (100, 20) in eval(): the buffer is the module's own flat arena, its parameters are views of it."""
    from hypad_amd.models import tadgan
    S, L = 100, 20

    def case(name, make, in_dim, out_dim):
        def build(seed):
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(seed)
                arena = make()._arena.clone()
            g = _gen(seed)
            return dict(x=torch.randn(ROWS, in_dim, generator=g), arena=arena, go=torch.randn(1, ROWS, out_dim, generator=g))

        def place(host):
            m = make().cuda().eval()
            ops = dict(x=torch.empty(ROWS, in_dim, device="cuda"), arena=m.arena(), go=torch.empty(1, ROWS, out_dim, device="cuda"), _module=m)
            assert ops["arena"].shape == host["arena"].shape
            return ops

        def run(ops):
            m, x = ops["_module"], _leaf(ops["x"])
            res = m(x)
            res = res if isinstance(res, tuple) else (res,)
            return [*(r.detach() for r in res), *torch.autograd.grad(res[0], [x, *m.parameters()], ops["go"])]
        return Case(name, build, run, place)
    return [case("tadgan.Encoder(100, 20), eval", lambda: tadgan.Encoder(S, L), S, L),
            case("tadgan.Decoder(100, 20, hyperbolic), eval", lambda: tadgan.Decoder(S, L, True), L, S),
            case("tadgan.CriticX(100, 20), eval", lambda: tadgan.CriticX(S, L), S, 1)]


# ------------------------------------------------------------------------------------------------ optim
def _optim_cases():
    from hypad_amd import optim
    from hypad_amd.hyperspace import hyrnn_nets as hn

    def build(seed):
        g = _gen(seed)
        return dict(ball=_ball(g, 1, 100, radius=0.6)[0], ball_grad=torch.randn(100, generator=g), ball_m=0.1 * torch.randn(100, generator=g),
                    ball_v=0.01 * torch.rand(100, generator=g) + 1e-4, w=torch.randn(17, 33, generator=g), w_grad=torch.randn(17, 33, generator=g),
                    w_m=0.1 * torch.randn(17, 33, generator=g), w_v=0.01 * torch.rand(17, 33, generator=g) + 1e-4)

    def run(cls, ops):
        """The third step from a given state: the parameter, gradient and both moments are the case's buffers; updated in place."""
        ball = hn.ManifoldParameter(ops["ball"], manifold=hn.PoincareBall())
        w = torch.nn.Parameter(ops["w"])
        opt = cls([ball, w], lr=1e-2, weight_decay=1e-3)
        opt.param_groups[0]["step"] = 2
        for p, n in ((ball, "ball"), (w, "w")):
            p.grad = ops[n + "_grad"]
            opt.state[p] = dict(step=2, exp_avg=ops[n + "_m"], exp_avg_sq=ops[n + "_v"])
        opt.step()
        return [ops[n] for n in ("ball", "ball_m", "ball_v", "w", "w_m", "w_v")]
    return [Case("optim.Adam", build, lambda ops: run(optim.Adam, ops), graph=False),
            Case("optim.RiemannianAdam", build, lambda ops: run(optim.RiemannianAdam, ops), graph=False)]


def cases():
    return _gmath_cases() + _hyrnn_cases() + _autograd_cases() + _module_cases() + _optim_cases()


# (the names alone, for parametrisation at collection time without importing the package)
NAMES = [
    "gmath.expmap0", "gmath.logmap0", "gmath.project", "gmath.mobius_fn_apply(tanh)", "gmath.mobius_add", "gmath.mobius_add, y of one row",
    "gmath.mobius_pointwise_mul", "gmath.mobius_pointwise_mul, w of one row", "gmath.poincare_rowdist", "gmath.hyperbolic_loss",
    "gmath.mobius_matvec 33->63", "gmath.dist2plane(signed, scaled)", "poincare_distance 65x130",
    "mobius_linear 33->63, Euclidean input, ball bias", "mobius_linear 33->63, ball input, ball bias, tanh",
    "mobius_linear 33->63, ball input, Euclidean bias", "mobius_linear 33->63, Euclidean input, Euclidean bias",
    "MobiusDist2Hyperplane(33, 17)", "mobius_gru_cell (17, 33, 63)", "mobius_gru_loop T = 3 (17, 33, 63)",
    "mobius_gru_loop batch_sizes [9, 7, 7, 4]", "autograd.linear_act 33->17, none", "autograd.linear_act 33->17, tanh",
    "autograd.linear_act 33->17, leaky", "autograd.lstm_layer 20->2x32, 39 rows (streamed)",
    "autograd.lstm_layer 100->2x50, 2053 rows (weights-stationary, saved gates)", "autograd.lstm_seq T = 3, 21 rows, 9->2x33, with h0 and c0",
    "tadgan.Encoder(100, 20), eval", "tadgan.Decoder(100, 20, hyperbolic), eval", "tadgan.CriticX(100, 20), eval",
    "optim.Adam", "optim.RiemannianAdam"]
OPTIMISERS = ("optim.Adam", "optim.RiemannianAdam")
