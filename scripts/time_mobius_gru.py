#!/usr/bin/env python3
"""Time forward + backward of hyrnn_nets.mobius_gru_loop against the plain-torch restatement (tests/mobius_gru_ref.py) run eagerly on the
device, at 64 rows x 100 steps of in = hidden = 100, ball-valued input and h0, no non-linearity.  HIP events, 5 warm-up runs, the median
and min .. max of 20.  Prints one JSON line.  Nothing depends on the figures; docs/history/mobius_gru.md records them.

    python scripts/time_mobius_gru.py
"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from hypad_amd.hyperspace import hyrnn_nets  # noqa: E402
from mobius_gru_ref import gru_loop_ref  # noqa: E402

ROWS, STEPS, I, H = 64, 100, 100, 100
WARMUP, RUNS = 5, 20


def ball(g, *shape, radius=0.8):
    a = torch.randn(*shape, generator=g)
    return a / a.norm(dim=-1, keepdim=True) * torch.rand(*shape[:-1], 1, generator=g) * radius


def timed(step):
    ms = []
    for i in range(WARMUP + RUNS):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        t1.synchronize()
        if i >= WARMUP:
            ms.append(t0.elapsed_time(t1))
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    g = torch.Generator().manual_seed(0)
    s = 1 / H ** 0.5
    host = (ball(g, STEPS, ROWS, I), ball(g, ROWS, H), (torch.rand(3 * H, I, generator=g) * 2 - 1) * s, (torch.rand(3 * H, H, generator=g) * 2 - 1) * s,
            ball(g, 3, H, radius=0.3))
    go = torch.randn(STEPS, ROWS, H, generator=g).cuda()
    ops = [t.cuda().requires_grad_(True) for t in host]

    def hip():
        outs, _ = hyrnn_nets.mobius_gru_loop(*ops, -1.0, hyperbolic_input=True, hyperbolic_hidden_state0=True)
        return torch.autograd.grad(outs, ops, go)

    def eager():
        outs, _, _ = gru_loop_ref(*ops)
        return torch.autograd.grad(outs, ops, go)

    a, b = hip(), eager()
    worst = max(float((u - v).abs().max()) / max(1.0, float(v.abs().max())) for u, v in zip(a, b))
    print(json.dumps(dict(shape=dict(rows=ROWS, steps=STEPS, in_dim=I, hidden=H), warmup=WARMUP, runs=RUNS, hip=timed(hip), torch_eager=timed(eager),
                          worst_gradient_difference=worst, device=torch.cuda.get_device_name(0))))


if __name__ == "__main__":
    main()
