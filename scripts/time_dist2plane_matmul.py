#!/usr/bin/env python3
"""Time dist2plane_matmul's HIP kernels against the plain-torch restatement (tests/dist2plane_matmul_ref.py) run eagerly in fp32 on the
same device, at the shape of a per-batch-element read-out: batch 64, N = M = 100, D = 64,
``dist2plane_matmul(x, points.transpose(-1, -2), normals.transpose(-1, -2))``, forward alone (no_grad) and forward + backward (the three
gradients).  The method of scripts/time_dist_matmul.py: HIP events around ``--inner`` back-to-back calls; 5 warm-ups of every variant,
then 20 samples per variant taken in alternation (hip, torch, hip, torch, ...) so that a drift of the machine hits both; the median and
the spread (min .. max) per call are printed, and one JSON line at the end.  The figures are call times: they include the enqueue.
Needs the GPU: there is no host fall-back.

    python scripts/time_dist2plane_matmul.py [--inner 200] [--samples 20] [--warmup 5]
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

from time_dist_matmul import ball, sample  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_dist2plane_matmul.py measures on the GPU; none is visible")
    from dist2plane_matmul_ref import dist2plane_matmul_ref
    from hypad_amd.hyperspace import gmath
    g = torch.Generator().manual_seed(0)
    x = ball(g, (64, 100, 64), 0.8).cuda()
    points = ball(g, (64, 100, 64), 0.8).cuda()
    normals = torch.randn(64, 100, 64, generator=g).cuda()
    go = torch.randn(64, 100, 100, generator=g).cuda()

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

    hip = lambda a, b, c: gmath.dist2plane_matmul(a, b.transpose(-1, -2), c.transpose(-1, -2), k=-1.0)
    ref = lambda a, b, c: dist2plane_matmul_ref(a, b.transpose(-1, -2), c.transpose(-1, -2))
    ops = (x, points, normals)
    cases = {"read-out fwd": (fwd(hip, *ops), fwd(ref, *ops)), "read-out fwd+bwd": (fwd_bwd(hip, go, *ops), fwd_bwd(ref, go, *ops))}
    # the two compute the same thing at this shape (fp32 against fp32), and each against the restatement in fp64 on the device: whose
    # rounding the difference between the two is
    with torch.no_grad():
        o_hip, o_ref, o_64 = hip(*ops), ref(*ops), ref(*(t.double() for t in ops))
        d, d_hip, d_ref = (float(t.abs().max()) for t in (o_hip - o_ref, o_hip.double() - o_64, o_ref.double() - o_64))
    print(f"max |hip - torch|: {d:.2e}   max |hip - fp64|: {d_hip:.2e}   max |torch - fp64|: {d_ref:.2e}   (max |out| {float(o_64.abs().max()):.2f})")
    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "max_abs_diff": d, "max_abs_diff_hip_fp64": d_hip,
              "max_abs_diff_torch_fp64": d_ref, "us_per_call": {}}
    for name, (h, r) in cases.items():
        for _ in range(args.warmup):
            sample(h, args.inner), sample(r, args.inner)
        th, tr = [], []
        for _ in range(args.samples):
            th.append(sample(h, args.inner))
            tr.append(sample(r, args.inner))
        mh, mr = statistics.median(th), statistics.median(tr)
        print(f"{name:20s} hip {mh:9.1f} us ({min(th):.1f} .. {max(th):.1f})   torch eager {mr:9.1f} us ({min(tr):.1f} .. {max(tr):.1f})   ratio {mr / mh:.2f}")
        result["us_per_call"][name] = {"hip": mh, "hip_min": min(th), "hip_max": max(th), "torch": mr, "torch_min": min(tr), "torch_max": max(tr)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
