#!/usr/bin/env python3
"""Time a whole training step -- zero_grad, forward, cross-entropy, backward, optimiser step -- of three models built from the library's
parts, under RiemannianAdam(manifold_rows=True), three ways (docs/history/capturable_optim.md):

    (a) eager, capturable=False: one launch per parameter, the step number by value -- the path as it was before the option existed;
    (b) eager, capturable=True: one advance launch and one grouped launch per 32 parameters, the step number on the device;
    (c) a replay of the step (b) captured into one graph;

and the optimiser part alone (``opt.step()`` on gradients that are in place) for (a) and (b).  The models, at 64 rows:
``head`` MobiusDist2Hyperplane(20, 6), three parameters; ``gru`` mobius_gru_loop (T = 8, 20 -> 20) -> MobiusDist2Hyperplane(20, 6), six;
``deep`` two stacked GRUs, two MobiusLinear(20, 20) and the read-out, thirteen.  The method of scripts/time_tangent_maps.py: HIP events
around ``--inner`` back-to-back steps, ``--warmup`` warm-ups of every variant, then ``--samples`` samples per variant taken in
alternation so that a drift of the machine hits all of them; the median and the spread (min .. max) per step in microseconds, and one
JSON line at the end.  The eager figures include the enqueue through Python: that is what a user's loop pays.

``--kernel`` adds the grouped kernel against hypad_radam_rows_step on one ball parameter of 10^6 rows of 32 under Adam, through the C
ABI; ``--bits`` compares the bits of a grouped launch with those of the per-parameter entry points on the same rows, for every kind, at
D = 1 .. 256 and steps 1 and 10.  Needs the GPU: there is no host fall-back.

    python scripts/time_train_step_graph.py [--inner 10] [--samples 20] [--warmup 5] [--kernel] [--bits]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)

from time_tangent_maps import ball, sample  # noqa: E402

ROWS, T, WIDTH, CLASSES = 64, 8, 20, 6
LR, B1, B2, EPS, WD, MU = 1e-3, 0.9, 0.999, 1e-8, 1e-5, 0.9


def models():
    from hypad_amd.hyperspace import hyrnn_nets as hn

    class GRU(torch.nn.Module):
        def __init__(self, g, hyperbolic_input):
            super().__init__()
            uni = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1) * WIDTH ** -0.5
            self.weight_ih, self.weight_hh = torch.nn.Parameter(uni(3 * WIDTH, WIDTH)), torch.nn.Parameter(uni(3 * WIDTH, WIDTH))
            self.bias = hn.ManifoldParameter(ball(g, (3, WIDTH), 0.5), manifold=hn.PoincareBall())
            self.register_buffer("h0", torch.zeros(ROWS, WIDTH))
            self.hyperbolic_input = hyperbolic_input

        def forward(self, x):
            return hn.mobius_gru_loop(x, self.h0, self.weight_ih, self.weight_hh, self.bias, -1.0, hyperbolic_input=self.hyperbolic_input)

    class Head(torch.nn.Module):
        def __init__(self, g):
            super().__init__()
            self.head = hn.MobiusDist2Hyperplane(WIDTH, CLASSES)

        def forward(self, x):
            return self.head(x)

    class Seq(torch.nn.Module):
        def __init__(self, g):
            super().__init__()
            self.gru, self.head = GRU(g, False), hn.MobiusDist2Hyperplane(WIDTH, CLASSES)

        def forward(self, x):
            return self.head(self.gru(x)[1])

    class Deep(torch.nn.Module):
        def __init__(self, g):
            super().__init__()
            self.gru1, self.gru2 = GRU(g, False), GRU(g, True)
            self.lin1, self.lin2 = hn.MobiusLinear(WIDTH, WIDTH, fp64_hyper=False), hn.MobiusLinear(WIDTH, WIDTH, fp64_hyper=False)
            self.head = hn.MobiusDist2Hyperplane(WIDTH, CLASSES)

        def forward(self, x):
            return self.head(self.lin2(self.lin1(self.gru2(self.gru1(x)[0])[1])))

    def build(cls):
        def make():
            torch.manual_seed(0)                                   # (the modules' own initialisation)
            return cls(torch.Generator().manual_seed(0)).cuda()
        return make
    g = torch.Generator().manual_seed(1)
    flat, seq = ball(g, (ROWS, WIDTH)).cuda(), (0.5 * torch.randn(T, ROWS, WIDTH, generator=g)).cuda()
    target = torch.randint(0, CLASSES, (ROWS,), generator=g).cuda()
    return {"head": (build(Head), flat, target), "gru": (build(Seq), seq, target), "deep": (build(Deep), seq, target)}


def train_step(model, opt, x, y):
    opt.zero_grad(set_to_none=True)
    torch.nn.functional.cross_entropy(model(x), y).backward()
    opt.step()


def time_models(args, result):
    from hypad_amd import optim
    for name, (make, x, y) in models().items():
        runs = {}
        for key, cap in (("a", False), ("b", True), ("c", True)):
            model = make()
            opt = optim.RiemannianAdam(model.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, stabilize=10, manifold_rows=True,
                                       capturable=cap)
            runs[key] = (model, opt)
        n_params = sum(1 for _ in runs["a"][0].parameters())
        fns = {"a whole step, eager, capturable off": lambda m=runs["a"]: train_step(*m, x, y),
               "b whole step, eager, capturable on": lambda m=runs["b"]: train_step(*m, x, y)}
        model, opt = runs["c"]
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(3):
                train_step(model, opt, x, y)
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            train_step(model, opt, x, y)
        fns["c whole step, one graph replay"] = graph.replay
        for key in ("a", "b"):                                     # the optimiser alone: the gradients of the last whole step stay in place
            fns[f"{key} optimiser step alone"] = runs[key][1].step
        for _ in range(args.warmup):
            for fn in fns.values():
                sample(fn, args.inner)
        times = {k: [] for k in fns}
        for _ in range(args.samples):
            for k, fn in fns.items():
                times[k].append(sample(fn, args.inner))
        print(f"{name}: {n_params} parameters, {ROWS} rows")
        entry = {"parameters": n_params}
        for k, ts in times.items():
            med = statistics.median(ts)
            print(f"  {k:40s} {med:9.1f} us ({min(ts):.1f} .. {max(ts):.1f})", flush=True)
            entry[k] = {"median": med, "min": min(ts), "max": max(ts)}
        result["models"][name] = entry


def time_kernel(args, result):
    """One ball parameter of 10^6 rows of 32 under Adam: hypad_radam_rows_step against a grouped launch of that one tensor."""
    from hypad_amd import _C
    rows, D = 10 ** 6, 32
    g = torch.Generator().manual_seed(2)
    sets = []
    for _ in range(2):
        p, gr = ball(g, (rows, D)).cuda(), torch.randn(rows, D, generator=g).cuda()
        sets.append((p, gr, torch.zeros_like(p), torch.zeros_like(p)))
    s = _C.stream()
    p, gr, m, v = sets[0]
    per = lambda: _C.check(_C.lib.hypad_radam_rows_step(_C.ptr(p), _C.ptr(gr), _C.ptr(m), _C.ptr(v), rows, D, _C.MANIFOLD_BALL, 7, 1e-4, B1, B2, EPS, WD, 0, s))
    q, gq, mq, vq = sets[1]
    d = (_C.OptimTensor * 1)()
    d[0].param, d[0].grad, d[0].state0, d[0].state1 = q.data_ptr(), gq.data_ptr(), mq.data_ptr(), vq.data_ptr()
    d[0].rows, d[0].numel, d[0].dim, d[0].manifold = rows, rows * D, D, _C.MANIFOLD_BALL
    grp = lambda: _C.check(_C.lib.hypad_optim_group_adam(d, 1, None, 7, None, 1e-4, B1, B2, EPS, WD, 0, s))
    for _ in range(args.warmup):
        sample(per, args.inner), sample(grp, args.inner)
    tp, tg = [], []
    for _ in range(args.samples):
        tp.append(sample(per, args.inner))
        tg.append(sample(grp, args.inner))
    nbytes = 4 * rows * D * 7
    print(f"ball / Adam ({rows}, {D}), one launch:")
    for k, ts in (("hypad_radam_rows_step", tp), ("hypad_optim_group_adam", tg)):
        med = statistics.median(ts)
        print(f"  {k:40s} {med:9.1f} us ({min(ts):.1f} .. {max(ts):.1f})  {nbytes / med * 1e-3:7.1f} GB/s", flush=True)
        result["kernel"][k] = {"median": med, "min": min(ts), "max": max(ts)}


def compare_bits(result):
    """The grouped launch against the per-parameter entry points on the same rows: both inline the same row functions."""
    from hypad_amd import _C
    s = _C.stream()
    g = torch.Generator().manual_seed(3)
    differing = []
    cases = 0
    for D in (1, 2, 20, 63, 64, 65, 255, 256):
        for man, kind in (("ball", _C.MANIFOLD_BALL), ("sphere", _C.MANIFOLD_SPHERE), ("euclidean", _C.MANIFOLD_EUCLIDEAN)):
            x = ball(g, (7, D)) if man == "ball" else torch.randn(7, D, generator=g)
            if man == "sphere":
                x = x / x.norm(dim=-1, keepdim=True)
            gr, m = torch.randn(7, D, generator=g), 0.1 * torch.randn(7, D, generator=g)
            v = ((m * m).mean(1, keepdim=True) + 0.01 * torch.rand(7, 1, generator=g)).expand(7, D).contiguous()
            for rule in ("adam", "sgd", "sgd-nesterov", "sgd-plain"):
                if rule == "adam" and man == "euclidean":
                    continue                                       # (the per-parameter rows step has no plain Adam)
                for step in (1, 10):
                    outs = []
                    for grouped in (False, True):
                        X, G, M, V = (t.cuda() for t in (x, gr, m, v))
                        d = (_C.OptimTensor * 1)()
                        d[0].param, d[0].grad, d[0].rows, d[0].numel, d[0].dim, d[0].manifold = X.data_ptr(), G.data_ptr(), 7, 7 * D, D, kind
                        if rule == "adam":
                            d[0].state0, d[0].state1 = M.data_ptr(), V.data_ptr()
                            rc = (_C.lib.hypad_optim_group_adam(d, 1, None, step, None, 0.05, B1, B2, EPS, 0.1, 10, s) if grouped else
                                  _C.lib.hypad_radam_rows_step(_C.ptr(X), _C.ptr(G), _C.ptr(M), _C.ptr(V), 7, D, kind, step, 0.05, B1, B2, EPS, 0.1, 10, s))
                        else:
                            mu, nest = (0.0 if rule == "sgd-plain" else MU), int(rule == "sgd-nesterov")
                            if mu:
                                d[0].state0 = M.data_ptr()
                            rc = (_C.lib.hypad_optim_group_sgd(d, 1, None, step, None, 0.05, mu, 0.0, 0.1, nest, 10, s) if grouped else
                                  _C.lib.hypad_rsgd_rows_step(_C.ptr(X), _C.ptr(G), _C.ptr(M) if mu else None, 7, D, kind, step, 0.05, mu, 0.0, 0.1, nest, 10, s))
                        _C.check(rc)
                        torch.cuda.synchronize()
                        outs.append((X.cpu(), M.cpu(), V.cpu()))
                    cases += 1
                    for name, a, b in zip(("p", "state0", "state1"), *outs):
                        if not torch.equal(a, b):
                            bad = (a != b).nonzero()
                            differing.append(f"{man} {rule} D {D} step {step}: {name} differs in {len(bad)} elements, first at {bad[0].tolist()}, "
                                             f"max |diff| {float((a - b).abs().max()):.3e}")
    print(f"grouped launch against the per-parameter entry points: {cases} cases, {len(differing)} tensors with differing bits")
    for line in differing:
        print("  " + line)
    result["bits"] = {"cases": cases, "differing": differing}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--bits", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_train_step_graph.py measures on the GPU; none is visible")
    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "models": {}, "kernel": {}}
    time_models(args, result)
    if args.kernel:
        time_kernel(args, result)
    if args.bits:
        compare_bits(result)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
