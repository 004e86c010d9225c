#!/usr/bin/env python3
"""Time gmath.hyperbolic_attention (one fused HIP launch forward, three backward) against the composition of the library's own
``dist_matmul``, ``torch.softmax`` and ``weighted_midpoint_bmm`` on the same device, at two shapes: batch 64, N = M = 100, D = E = 64,
and batch 8, N = M = 1024, D = E = 64; forward alone (no_grad) and forward + backward.  HIP events around ``--inner`` back-to-back calls;
``--warmup`` warm-ups of every variant, then ``--samples`` samples per variant taken in alternation (fused, composed, fused, ...) so that
a drift of the machine hits both; the median and the spread (min .. max) per call are printed, and one JSON line at the end.  The
figures are call times through the Python functions: they include the enqueue.  Needs the GPU: there is no host fall-back.

    python scripts/time_hyperbolic_attention.py [--inner 50] [--samples 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BETA = 1.7
SHAPES = ((64, 100, 100, 64, 64), (8, 1024, 1024, 64, 64))      # (batch, N, M, D, E)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hyperbolic_attention.py measures on the GPU; none is visible")
    from hypad_amd.hyperspace import gmath

    fused = lambda q, k, v: gmath.hyperbolic_attention(q, k, v, -1.0, beta=BETA)
    composed = lambda q, k, v: gmath.weighted_midpoint_bmm(v, torch.softmax(-BETA * gmath.dist_matmul(q, k.transpose(-1, -2), -1.0), -1), -1.0)

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

    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "beta": BETA, "shapes": {}}
    for shape in SHAPES:
        batch, N, M, D, E = shape
        g = torch.Generator().manual_seed(0)
        q, keys, values = ball(g, (batch, N, D)).cuda(), ball(g, (batch, M, D)).cuda(), ball(g, (batch, M, E)).cuda()
        go = torch.randn(batch, N, E, generator=g).cuda()
        with torch.no_grad():
            d = float((fused(q, keys, values) - composed(q, keys, values)).abs().max())
        print(f"{shape}: max |fused - composed| {d:.2e}")
        entry = {"max_abs_diff": d}
        cases = {"fwd": (fwd(fused, q, keys, values), fwd(composed, q, keys, values)),
                 "fwd+bwd": (fwd_bwd(fused, go, q, keys, values), fwd_bwd(composed, go, q, keys, values))}
        for name, (f, c) in cases.items():
            for _ in range(args.warmup):
                sample(f, args.inner), sample(c, args.inner)
            tf, tc = [], []
            for _ in range(args.samples):
                tf.append(sample(f, args.inner))
                tc.append(sample(c, args.inner))
            mf, mc = statistics.median(tf), statistics.median(tc)
            print(f"  {name:8s} fused {mf:9.1f} us ({min(tf):.1f} .. {max(tf):.1f})   composed {mc:9.1f} us ({min(tc):.1f} .. {max(tc):.1f})   "
                  f"composed / fused {mc / mf:.2f}")
            entry[name] = {"fused": mf, "fused_min": min(tf), "fused_max": max(tf), "composed": mc, "composed_min": min(tc), "composed_max": max(tc)}
        result["shapes"]["x".join(map(str, shape))] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
