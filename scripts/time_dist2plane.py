#!/usr/bin/env python3
"""Time MobiusDist2Hyperplane's forward + backward (hypad_dist2plane_*) against the same formula in torch eager on the device.

    python scripts/time_dist2plane.py [--rows 200000] [--k 100] [--n 100] [--runs 20] [--warmup 5]

HIP events around each forward + backward, a warm-up, the median of the runs; one JSON line.  Nothing is claimed from the figure: it
is recorded in docs/history/dist2plane.md.
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


def timed(step, runs, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=200000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from dist2plane_ref import layer_ref
    from hypad_amd.hyperspace import hyrnn_nets
    torch.manual_seed(0)
    layer = hyrnn_nets.MobiusDist2Hyperplane(args.k, args.n).cuda()
    x = torch.randn(args.rows, args.k, device="cuda")
    x = (x / x.norm(dim=1, keepdim=True) * (0.9 * torch.rand(args.rows, 1, device="cuda"))).requires_grad_(True)
    go = torch.randn(args.rows, args.n, device="cuda")
    params = [x] + list(layer.parameters())

    def clear():
        for t in params:
            t.grad = None

    def hip():
        clear()
        layer(x).backward(go)

    def eager():
        clear()
        layer_ref(x, layer.point, layer.tangent, layer.scale).backward(go)

    h, e = timed(hip, args.runs, args.warmup), timed(eager, args.runs, args.warmup)
    print(json.dumps(dict(rows=args.rows, k=args.k, n=args.n, runs=args.runs, hip_ms_median=round(h[0], 3), hip_ms_min=round(h[1], 3),
                          hip_ms_max=round(h[2], 3), eager_ms_median=round(e[0], 3), eager_ms_min=round(e[1], 3), eager_ms_max=round(e[2], 3),
                          eager_over_hip=round(e[0] / h[0], 2))))


if __name__ == "__main__":
    main()
