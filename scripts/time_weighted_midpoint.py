#!/usr/bin/env python3
"""Time the weighted Moebius gyromidpoint's HIP kernels against the plain-torch restatement (tests/midpoint_ref.py) run eagerly on the
same device, at the two shapes a user of the layers would run:

    attention   weighted_midpoint_bmm: batch 64, N = M = 100, D = 64 (softmax weights)
    pooling     weighted_midpoint over the steps of a GRU's output: 100 steps x 64 rows x H = 100 (positive weights per step and row)

each forward alone (no_grad) and forward + backward.  HIP events around ``--inner`` back-to-back calls; 5 warm-ups of every variant,
then 20 samples per variant taken in alternation (hip, torch, hip, torch, ...) so that a drift of the machine hits both; the median
and the spread (min .. max) per call are printed, and one JSON line at the end.  Needs the GPU: there is no host fall-back.

    python scripts/time_weighted_midpoint.py [--inner 200] [--samples 20] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_weighted_midpoint.py measures on the GPU; none is visible")
    from hypad_amd.hyperspace import gmath
    from midpoint_ref import weighted_midpoint_bmm_ref, weighted_midpoint_ref
    g = torch.Generator().manual_seed(0)
    xs = ball(g, (64, 100, 64)).cuda()
    w = torch.softmax(torch.randn(64, 100, 100, generator=g), dim=-1).cuda()
    go = torch.randn(64, 100, 64, generator=g).cuda()
    px = ball(g, (100, 64, 100)).cuda()
    pw = (0.1 + 0.9 * torch.rand(100, 64, generator=g)).cuda()
    pgo = torch.randn(64, 100, generator=g).cuda()

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

    hip_bmm = lambda a, b: gmath.weighted_midpoint_bmm(a, b, -1.0)
    ref_bmm = lambda a, b: weighted_midpoint_bmm_ref(a, b)
    hip_red = lambda a, b: gmath.weighted_midpoint(a, -1.0, weights=b, reducedim=[0])
    ref_red = lambda a, b: weighted_midpoint_ref(a, b, reducedim=[0])
    cases = {
        "attention fwd": (fwd(hip_bmm, xs, w), fwd(ref_bmm, xs, w)),
        "attention fwd+bwd": (fwd_bwd(hip_bmm, go, xs, w), fwd_bwd(ref_bmm, go, xs, w)),
        "pooling fwd": (fwd(hip_red, px, pw), fwd(ref_red, px, pw)),
        "pooling fwd+bwd": (fwd_bwd(hip_red, pgo, px, pw), fwd_bwd(ref_red, pgo, px, pw)),
    }
    # the two compute the same thing at these shapes (fp32 against fp32: reordered sums only)
    with torch.no_grad():
        d_bmm = float((hip_bmm(xs, w) - ref_bmm(xs, w)).abs().max())
        d_red = float((hip_red(px, pw) - ref_red(px, pw)).abs().max())
    print(f"max |hip - torch|: attention {d_bmm:.2e}, pooling {d_red:.2e}")
    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "max_abs_diff": {"attention": d_bmm, "pooling": d_red}, "us_per_call": {}}
    for name, (hip, ref) in cases.items():
        for _ in range(args.warmup):
            sample(hip, args.inner), sample(ref, args.inner)
        th, tr = [], []
        for _ in range(args.samples):
            th.append(sample(hip, args.inner))
            tr.append(sample(ref, args.inner))
        mh, mr = statistics.median(th), statistics.median(tr)
        print(f"{name:20s} hip {mh:9.1f} us ({min(th):.1f} .. {max(th):.1f})   torch eager {mr:9.1f} us ({min(tr):.1f} .. {max(tr):.1f})   ratio {mr / mh:.2f}")
        result["us_per_call"][name] = {"hip": mh, "hip_min": min(th), "hip_max": max(th), "torch": mr, "torch_min": min(tr), "torch_max": max(tr)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
