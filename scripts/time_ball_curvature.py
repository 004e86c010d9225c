#!/usr/bin/env python3
"""Time the methods of hyrnn_nets.PoincareBall(c) at c = 0.5 (the hypad_ball_* kernels: one HIP launch forward and one backward, the
curvature applied in registers) against the same ``gmath`` function at k = -1 (the kernels they share their templates with) and against
the composition a user writes without them, ``gmath.f(s x, ...) / s`` with s = sqrt(c) (docs/history/curvature.md has the exponents): for
expmap, logmap, mobius_add, dist, parallel_transport and inner at (10, 64), 6 400 x 64 and 10^6 x 32, forward alone (no_grad) and forward
+ backward.  The method of scripts/time_gyro_ops.py: HIP events around ``--inner`` back-to-back calls; ``--warmup`` warm-ups of every
variant, then ``--samples`` samples per variant taken in alternation so that a drift of the machine hits all three; the median and the
spread (min .. max) per call are printed, and one JSON line at the end.  The figures are call times through the Python functions: they
include the enqueue.  Needs the GPU: there is no host fall-back.

    python scripts/time_ball_curvature.py [--inner 50] [--samples 20] [--warmup 5]
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
SHAPES = ((10, 64), (64 * 100, 64), (10 ** 6, 32))      # (rows, D)


def variants(gmath, manifold):
    """name: (the method at c, gmath at k = -1 on the operands scaled onto the unit ball, the composition on the operands at c, kinds:
    p a point of the ball of radius 1 / sqrt(c), v a vector)."""
    s, k = math.sqrt(C), dict(k=-1.0)
    return {
        "expmap": (manifold.expmap, lambda x, u: gmath.expmap(x, u, **k), lambda x, u: gmath.expmap(s * x, s * u, **k) / s, "pv"),
        "logmap": (manifold.logmap, lambda x, y: gmath.logmap(x, y, **k), lambda x, y: gmath.logmap(s * x, s * y, **k) / s, "pp"),
        "mobius_add": (manifold.mobius_add, lambda x, y: gmath.mobius_add(x, y, **k), lambda x, y: gmath.mobius_add(s * x, s * y, **k) / s, "pp"),
        "dist": (manifold.dist, lambda x, y: gmath.dist(x, y, **k), lambda x, y: gmath.dist(s * x, s * y, **k) / s, "pp"),
        "parallel_transport": (manifold.parallel_transport, lambda x, y, v: gmath.parallel_transport(x, y, v, **k),
                               lambda x, y, v: gmath.parallel_transport(s * x, s * y, v, **k), "ppv"),
        "inner": (manifold.inner, lambda x, u, v: gmath.inner(x, u, v, **k), lambda x, u, v: gmath.inner(s * x, u, v, **k), "pvw"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_ball_curvature.py measures on the GPU; none is visible")
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

    result = {"c": C, "inner": args.inner, "samples": args.samples, "warmup": args.warmup, "shapes": {}}
    s = math.sqrt(C)
    for rows, D in SHAPES:
        g = torch.Generator().manual_seed(0)
        unit_pts = [ball(g, (rows, D)).cuda() for _ in range(2)]
        vecs = {"v": torch.randn(rows, D, generator=g).cuda(), "w": torch.randn(rows, D, generator=g).cuda()}
        shape_entry = {}
        print(f"({rows}, {D})")
        for name, (method, unit, composed, kinds) in variants(gmath, manifold).items():
            it = iter(unit_pts)
            on_unit = [next(it) if kind == "p" else vecs[kind] for kind in kinds]
            ops = [t / s if kind == "p" else t for t, kind in zip(on_unit, kinds)]
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
                print(f"  {name:18s} {case:8s} method(c) {med[0]:9.1f} us ({min(times[0]):.1f} .. {max(times[0]):.1f})   gmath(k=-1) {med[1]:9.1f} us "
                      f"({min(times[1]):.1f} .. {max(times[1]):.1f})   composed {med[2]:9.1f} us ({min(times[2]):.1f} .. {max(times[2]):.1f})   "
                      f"method / gmath {med[0] / med[1]:.2f}   composed / method {med[2] / med[0]:.2f}   max |method - composed| {d:.1e}", flush=True)
                entry[case] = {"method": med[0], "method_min": min(times[0]), "method_max": max(times[0]), "gmath_k1": med[1],
                               "gmath_k1_min": min(times[1]), "gmath_k1_max": max(times[1]), "composed": med[2], "composed_min": min(times[2]),
                               "composed_max": max(times[2])}
            shape_entry[name] = entry
        result["shapes"][f"{rows}x{D}"] = shape_entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
