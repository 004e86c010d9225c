#!/usr/bin/env python3
"""Time the tangent maps of hyperspace/gmath (expmap, logmap, geodesic, gyration, parallel_transport, parallel_transport0,
parallel_transport0back: one fused HIP launch forward and one backward each) against the same function composed from the library's
other ops (mobius_add, mobius_scalar_mul) and torch, on the same device, at two shapes: 64 * 100 rows of D = 64 and 10^6 rows of D = 32;
forward alone (no_grad) and forward + backward.  HIP events around ``--inner`` back-to-back calls; ``--warmup`` warm-ups of every
variant, then ``--samples`` samples per variant taken in alternation (fused, composed, fused, ...) so that a drift of the machine hits
both; the median and the spread (min .. max) per call are printed, with the bytes per second the fused median moves of the op's
algorithmic bytes -- every operand and gradient read or written once, 4 bytes an element --, and one JSON line at the end.  The figures
are call times through the Python functions: they include the enqueue.  Needs the GPU: there is no host fall-back.

    python scripts/time_tangent_maps.py [--inner 50] [--samples 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64 * 100, 64), (10 ** 6, 32))      # (rows, D)
T = 0.3


def ball(g, shape, radius=0.9):
    x = torch.randn(shape, generator=g)
    return x / x.norm(dim=-1, keepdim=True) * (torch.rand(shape[:-1] + (1,), generator=g) * radius)


def sample(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / inner          # us per call


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


def _conformal(x):
    return (1 - _dot(x, x)).clamp_min(1e-15)


def _artanh(n):
    n = n.clamp(-1 + 1e-7, 1 - 1e-7)
    return 0.5 * (torch.log1p(n) - torch.log1p(-n))


def _gyration(a, b, u):
    a2, b2, ab, au, bu = _dot(a, a), _dot(b, b), _dot(a, b), _dot(a, u), _dot(b, u)
    return u + 2 * ((-au * b2 + bu + 2 * ab * bu) * a + (-bu * a2 - au) * b) / (1 + 2 * ab + a2 * b2).clamp_min(1e-15)


def variants(gmath):
    """name: (fused, composed, the operands: p a point of the ball, v a vector)."""
    def c_expmap(x, u):
        n = u.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        return gmath.mobius_add(x, (n / _conformal(x)).clamp(-15, 15).tanh() * (u / n))

    def c_logmap(x, y):
        w = gmath.mobius_add(-x, y)
        n = w.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        return _artanh(n) * _conformal(x) * (w / n)

    k = dict(k=-1.0)
    return {
        "expmap": (lambda x, u: gmath.expmap(x, u, **k), c_expmap, "pv"),
        "logmap": (lambda x, y: gmath.logmap(x, y, **k), c_logmap, "pp"),
        "geodesic": (lambda x, y: gmath.geodesic(T, x, y, **k), lambda x, y: gmath.mobius_add(x, gmath.mobius_scalar_mul(T, gmath.mobius_add(-x, y))), "pp"),
        "gyration": (lambda a, b, u: gmath.gyration(a, b, u, **k), _gyration, "ppv"),
        "parallel_transport": (lambda x, y, v: gmath.parallel_transport(x, y, v, **k), lambda x, y, v: _gyration(y, -x, v) * (_conformal(y) / _conformal(x)), "ppv"),
        "parallel_transport0": (lambda y, v: gmath.parallel_transport0(y, v, **k), lambda y, v: v * _conformal(y), "pv"),
        "parallel_transport0back": (lambda x, v: gmath.parallel_transport0back(x, v, **k), lambda x, v: v / _conformal(x), "pv"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_tangent_maps.py measures on the GPU; none is visible")
    from hypad_amd.hyperspace import gmath

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

    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "t": T, "shapes": {}}
    for rows, D in SHAPES:
        g = torch.Generator().manual_seed(0)
        pts = [ball(g, (rows, D)).cuda() for _ in range(2)]
        vec = torch.randn(rows, D, generator=g).cuda()
        go = torch.randn(rows, D, generator=g).cuda()
        shape_entry = {}
        print(f"({rows}, {D})")
        for name, (fused, composed, kinds) in variants(gmath).items():
            n, points = len(kinds), iter(pts)
            ops = [next(points) if kind == "p" else vec for kind in kinds]
            with torch.no_grad():
                d = float((fused(*ops) - composed(*ops)).abs().max())
            entry = {"max_abs_diff": d}
            # every operand and the result once forward; operands, grad_out and every gradient once backward
            nbytes = {"fwd": 4 * rows * D * (n + 1), "fwd+bwd": 4 * rows * D * (n + 1 + 2 * n + 1)}
            cases = {"fwd": (fwd(fused, *ops), fwd(composed, *ops)), "fwd+bwd": (fwd_bwd(fused, go, *ops), fwd_bwd(composed, go, *ops))}
            for case, (f, c) in cases.items():
                for _ in range(args.warmup):
                    sample(f, args.inner), sample(c, args.inner)
                tf, tc = [], []
                for _ in range(args.samples):
                    tf.append(sample(f, args.inner))
                    tc.append(sample(c, args.inner))
                mf, mc = statistics.median(tf), statistics.median(tc)
                gbs = nbytes[case] / mf * 1e-3
                print(f"  {name:24s} {case:8s} fused {mf:9.1f} us ({min(tf):.1f} .. {max(tf):.1f})  {gbs:7.1f} GB/s   composed {mc:9.1f} us "
                      f"({min(tc):.1f} .. {max(tc):.1f})   composed / fused {mc / mf:.2f}   max |fused - composed| {d:.1e}")
                entry[case] = {"fused": mf, "fused_min": min(tf), "fused_max": max(tf), "composed": mc, "composed_min": min(tc), "composed_max": max(tc),
                               "algorithmic_bytes": nbytes[case], "fused_gb_per_s": gbs}
            shape_entry[name] = entry
        result["shapes"][f"{rows}x{D}"] = shape_entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
