#!/usr/bin/env python3
"""Time the gyrovector and metric ops of hyperspace/gmath (mobius_sub, mobius_coadd, mobius_cosub, geodesic_unit, lambda_x, inner, norm,
egrad2rgrad, sproj, inv_sproj: one fused HIP launch forward and one backward each) against the same function composed from the
library's other ops (mobius_add) and eager fp32 torch, on the same device, at two shapes: 64 * 100 rows of D = 64 and 10^6 rows of
D = 32; forward alone (no_grad) and forward + backward.  The method of scripts/time_tangent_maps.py: HIP events around ``--inner``
back-to-back calls; ``--warmup`` warm-ups of every variant, then ``--samples`` samples per variant taken in alternation (fused, composed,
fused, ...) so that a drift of the machine hits both; the median and the spread (min .. max) per call are printed, with the bytes per
second the fused median moves of the op's algorithmic bytes -- every operand and gradient read or written once, 4 bytes an element --,
and one JSON line at the end.  The figures are call times through the Python functions: they include the enqueue.  Needs the GPU: there
is no host fall-back.

    python scripts/time_gyro_ops.py [--inner 50] [--samples 20] [--warmup 5]
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

from time_tangent_maps import SHAPES, _conformal, _dot, ball, sample  # noqa: E402

T = 0.7


def _coadd(x, y):
    x2, y2 = _dot(x, x), _dot(y, y)
    return ((1 - y2) * x + (1 - x2) * y) / (1 - x2 * y2).clamp_min(1e-15)


def _inv_sproj(x):
    lam = 2 / _conformal(x)
    return torch.cat((lam * x, lam - 1), dim=-1)


def variants(gmath):
    """name: (fused, composed, the operands: p a point of the ball, v and w vectors, h a point of the hyperboloid, one column wider)."""
    def c_geodesic_unit(x, u):
        return gmath.mobius_add(x, math.tanh(T / 2) * (u / u.norm(dim=-1, keepdim=True).clamp_min(1e-15)))

    k = dict(k=-1.0)
    return {
        "mobius_sub": (lambda x, y: gmath.mobius_sub(x, y, **k), lambda x, y: gmath.mobius_add(x, -y), "pp"),
        "mobius_coadd": (lambda x, y: gmath.mobius_coadd(x, y, **k), _coadd, "pp"),
        "mobius_cosub": (lambda x, y: gmath.mobius_cosub(x, y, **k), lambda x, y: _coadd(x, -y), "pp"),
        "geodesic_unit": (lambda x, u: gmath.geodesic_unit(T, x, u, **k), c_geodesic_unit, "pv"),
        "lambda_x": (lambda x: gmath.lambda_x(x, **k), lambda x: (2 / _conformal(x)).squeeze(-1), "p"),
        "inner": (lambda x, u, v: gmath.inner(x, u, v, **k), lambda x, u, v: ((2 / _conformal(x)) ** 2 * _dot(u, v)).squeeze(-1), "pvw"),
        "norm": (lambda x, u: gmath.norm(x, u, **k), lambda x, u: (2 / _conformal(x)).squeeze(-1) * u.norm(dim=-1), "pv"),
        "egrad2rgrad": (lambda x, g: gmath.egrad2rgrad(x, g, **k), lambda x, g: g / (2 / _conformal(x)) ** 2, "pv"),
        "sproj": (lambda h: gmath.sproj(h, **k), lambda h: h[..., :-1] / (1 + h[..., -1:]), "h"),
        "inv_sproj": (lambda x: gmath.inv_sproj(x, **k), _inv_sproj, "p"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_gyro_ops.py measures on the GPU; none is visible")
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
        data = {"v": torch.randn(rows, D, generator=g).cuda(), "w": torch.randn(rows, D, generator=g).cuda()}
        with torch.no_grad():
            data["h"] = _inv_sproj(pts[1].double()).float()
        shape_entry = {}
        print(f"({rows}, {D})")
        for name, (fused, composed, kinds) in variants(gmath).items():
            points = iter(pts)
            ops = [next(points) if kind == "p" else data[kind] for kind in kinds]
            with torch.no_grad():
                out = fused(*ops)
                d = float((out - composed(*ops)).abs().max() / out.abs().max().clamp_min(1.0))
            go = torch.randn(out.shape, generator=g).cuda()
            entry = {"max_rel_diff": d}
            # every operand and the result once forward; operands, grad_out and every gradient once backward
            n_in = sum(t.numel() for t in ops)
            nbytes = {"fwd": 4 * (n_in + out.numel()), "fwd+bwd": 4 * (n_in + out.numel() + 2 * n_in + out.numel())}
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
                print(f"  {name:16s} {case:8s} fused {mf:9.1f} us ({min(tf):.1f} .. {max(tf):.1f})  {gbs:7.1f} GB/s   composed {mc:9.1f} us "
                      f"({min(tc):.1f} .. {max(tc):.1f})   composed / fused {mc / mf:.2f}   max |fused - composed| / max(1, max|fused|) {d:.1e}",
                      flush=True)
                entry[case] = {"fused": mf, "fused_min": min(tf), "fused_max": max(tf), "composed": mc, "composed_min": min(tc), "composed_max": max(tc),
                               "algorithmic_bytes": nbytes[case], "fused_gb_per_s": gbs}
            shape_entry[name] = entry
        result["shapes"][f"{rows}x{D}"] = shape_entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
