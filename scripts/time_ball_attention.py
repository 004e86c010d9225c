#!/usr/bin/env python3
"""Time the matmul methods of hyrnn_nets.PoincareBall(c) at c = 0.5 -- dist_matmul, weighted_midpoint_bmm, weighted_midpoint and
hyperbolic_attention, the hypad_ball_* instantiations of the k = -1 kernels with c in their fp64 stages (docs/history/curvature_matmul.md)
-- against the same ``gmath`` function at k = -1 on operands scaled onto the unit ball beforehand, and against the composition a user
writes without the methods, ``gmath.f(s x, ...) / s`` with s = sqrt(c), which for attention is
``gmath.hyperbolic_attention(s q, s keys, s values, -1, beta / s) / s``.  Shapes (batch, N, M, D) with E = D: (32, 100, 100, 64), where a
call is bound by its enqueue, and (8, 1024, 1024, 64), the shape csrc/attention.hip cites for its tuning; the pooling form reduces 100
positions of 6 400 rows of 64.  Forward alone (no_grad) and forward + backward.  The method of scripts/time_ball_curvature.py: HIP events
around ``--inner`` back-to-back calls; ``--warmup`` warm-ups of every variant, then ``--samples`` samples per variant taken in alternation
so that a drift of the machine hits all three; the median and the spread (min .. max) per call are printed, and one JSON line at the end.
The figures are call times through the Python functions: they include the enqueue.  Needs the GPU: there is no host fall-back.

    python scripts/time_ball_attention.py [--inner 50] [--samples 20] [--warmup 5]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, ROOT)

from time_tangent_maps import ball, sample  # noqa: E402

C = 0.5
BETA = 1.7
SHAPES = ((32, 100, 100, 64), (8, 1024, 1024, 64))      # (batch, N, M, D), E = D
REDUCE_SHAPE = (100, 64 * 100, 64)                      # (positions, rows, D)


def variants(gmath, manifold):
    """name: (the method at c, gmath at k = -1 on operands that are on the unit ball already, the composition on the operands at c)."""
    s = math.sqrt(C)
    return {
        "dist_matmul": (lambda x, y: manifold.dist_matmul(x, y.transpose(-1, -2)), lambda x, y: gmath.dist_matmul(x, y.transpose(-1, -2), -1.0),
                        lambda x, y: gmath.dist_matmul(s * x, (s * y).transpose(-1, -2), -1.0) / s),
        "weighted_midpoint_bmm": (lambda xs, w: manifold.weighted_midpoint_bmm(xs, w), lambda xs, w: gmath.weighted_midpoint_bmm(xs, w, -1.0),
                                  lambda xs, w: gmath.weighted_midpoint_bmm(s * xs, w, -1.0) / s),
        "hyperbolic_attention": (lambda q, k, v: manifold.hyperbolic_attention(q, k, v, beta=BETA),
                                 lambda q, k, v: gmath.hyperbolic_attention(q, k, v, -1.0, beta=BETA / s),
                                 lambda q, k, v: gmath.hyperbolic_attention(s * q, s * k, s * v, -1.0, beta=BETA / s) / s),
        "weighted_midpoint": (lambda xs: manifold.weighted_midpoint(xs, reducedim=[0]), lambda xs: gmath.weighted_midpoint(xs, -1.0, reducedim=[0]),
                              lambda xs: gmath.weighted_midpoint(s * xs, -1.0, reducedim=[0]) / s),
    }


def operands(name, shape, g):
    """(the operands on the unit ball, which of them are points)."""
    if name == "weighted_midpoint":
        return [ball(g, shape).cuda()], [True]
    batch, N, M, D = shape
    if name == "dist_matmul":
        return [ball(g, (batch, N, D)).cuda(), ball(g, (batch, M, D)).cuda()], [True, True]
    if name == "weighted_midpoint_bmm":
        return [ball(g, (batch, M, D)).cuda(), torch.softmax(torch.randn(batch, N, M, generator=g), -1).cuda()], [True, False]
    return [ball(g, (batch, N, D)).cuda(), ball(g, (batch, M, D)).cuda(), ball(g, (batch, M, D)).cuda()], [True, True, True]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ball_attention.py measures on the GPU; none is visible")
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace.hyrnn_nets import PoincareBall
    manifold = PoincareBall(C)

    def fwd(f, *ops):
        def run():
            with torch.no_grad():
                f(*ops)
        return run

    def fwd_bwd(f, grad_out, *ops):
        leaves = [t.clone().requires_grad_(True) for t in ops]

        def run():
            torch.autograd.grad(f(*leaves), leaves, grad_out)
        return run

    result = {"c": C, "beta": BETA, "inner": args.inner, "samples": args.samples, "warmup": args.warmup, "shapes": {}}
    s = math.sqrt(C)
    table = variants(gmath, manifold)
    todo = [(shape, n) for shape in SHAPES for n in ("dist_matmul", "weighted_midpoint_bmm", "hyperbolic_attention")] + [(REDUCE_SHAPE, "weighted_midpoint")]
    for shape, name in todo:
        method, unit, composed = table[name]
        g = torch.Generator().manual_seed(0)
        on_unit, is_point = operands(name, shape, g)
        ops = [t / s if p else t for t, p in zip(on_unit, is_point)]
        with torch.no_grad():
            out = method(*ops)
            d = float((out - composed(*ops)).abs().max() / out.abs().max().clamp_min(1.0))
        go = torch.randn(out.shape, generator=g).cuda()
        entry = {"max_rel_diff": d}
        cases = {"fwd": [fwd(method, *ops), fwd(unit, *on_unit), fwd(composed, *ops)],
                 "fwd+bwd": [fwd_bwd(method, go, *ops), fwd_bwd(unit, go, *on_unit), fwd_bwd(composed, go, *ops)]}
        for case, runs in cases.items():
            for _ in range(args.warmup):
                for r in runs:
                    sample(r, args.inner)
            times = [[], [], []]
            for _ in range(args.samples):
                for t, r in zip(times, runs):
                    t.append(sample(r, args.inner))
            med = [statistics.median(t) for t in times]
            print(f"{str(shape):22s} {name:22s} {case:8s} method(c) {med[0]:9.1f} us ({min(times[0]):.1f} .. {max(times[0]):.1f})   gmath(k=-1) {med[1]:9.1f} us "
                  f"({min(times[1]):.1f} .. {max(times[1]):.1f})   composed {med[2]:9.1f} us ({min(times[2]):.1f} .. {max(times[2]):.1f})   "
                  f"method / gmath {med[0] / med[1]:.2f}   composed / method {med[2] / med[0]:.2f}   max |method - composed| {d:.1e}", flush=True)
            entry[case] = {"method": med[0], "method_min": min(times[0]), "method_max": max(times[0]), "gmath_k1": med[1],
                           "gmath_k1_min": min(times[1]), "gmath_k1_max": max(times[1]), "composed": med[2], "composed_min": min(times[2]),
                           "composed_max": max(times[2])}
        result["shapes"].setdefault("x".join(map(str, shape)), {})[name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
