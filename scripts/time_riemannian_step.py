#!/usr/bin/env python3
"""Time one row-wise Riemannian optimiser step -- RiemannianAdam(manifold_rows=True) and RiemannianSGD(momentum=0.9) on a PoincareBall
and on a Sphere parameter, one HIP launch each (csrc/riemann_opt.hip) -- against the same rule composed from what the library offered
before it: gmath.egrad2rgrad, inner, project, parallel_transport and torch's elementwise ops for the ball, torch ops for the sphere, on
the same device.  Three shapes: MobiusDist2Hyperplane's own scale (10, 64), and the two of the earlier documents, 64 * 100 rows of
D = 64 and 10^6 rows of D = 32.  The method of scripts/time_tangent_maps.py: HIP events around ``--inner`` back-to-back steps;
``--warmup`` warm-ups of every variant, then ``--samples`` samples per variant taken in alternation (fused, composed, fused, ...) so
that a drift of the machine hits both; the median and the spread (min .. max) per step are printed, with the bytes per second the fused
median moves of the step's algorithmic bytes -- the parameter and every state tensor read and written once, the gradient read once, 4
bytes an element --, and one JSON line at the end.  The figures are step times through the Python classes: they include the enqueue.
Both sides step the same kind of state in place for the whole run (lr 1e-4, one fixed gradient), from equal starts; the first step of
each is compared.  Needs the GPU: there is no host fall-back.

    python scripts/time_riemannian_step.py [--inner 50] [--samples 20] [--warmup 5]
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

from time_tangent_maps import _dot, ball, sample  # noqa: E402

SHAPES = ((10, 64), (64 * 100, 64), (10 ** 6, 32))      # (rows, D)
LR, B1, B2, EPS, WD, MU = 1e-4, 0.9, 0.999, 1e-8, 1e-5, 0.9
K = dict(k=-1.0)


class Composed:
    """The rules of docs/history/riemannian_rows.md out of library ops and torch, stepping p and its state in place."""

    def __init__(self, gmath, man, rule, p, g):
        self.gmath, self.man, self.rule, self.p, self.g, self.t = gmath, man, rule, p, g, 0
        self.m, self.v = torch.zeros_like(p), torch.zeros_like(p)
        self.buf = None

    def rgrad(self, x, g):
        return self.gmath.egrad2rgrad(x, g, **K) if self.man == "ball" else g - _dot(x, g) * x

    def retr(self, x, u):
        if self.man == "ball":
            return self.gmath.project(x + u, **K)
        y = x + u
        return y / y.norm(dim=-1, keepdim=True).clamp_min(1e-15)

    def transp(self, x, y, w):
        return self.gmath.parallel_transport(x, y, w, **K) if self.man == "ball" else w - _dot(y, w) * y

    @torch.no_grad()
    def step(self):
        self.t += 1
        p, t = self.p, self.t
        g = self.g.add(p, alpha=WD)
        r = self.rgrad(p, g)
        if self.rule == "adam":
            s = self.gmath.inner(p, r, r, keepdim=True, **K) if self.man == "ball" else _dot(r, r)
            self.m.mul_(B1).add_(r, alpha=1 - B1)
            self.v.mul_(B2).add_(s * (1 - B2))
            d = (self.m / (1 - B1 ** t)) / ((self.v / (1 - B2 ** t)).sqrt() + EPS)
            w = self.m
        else:
            if self.buf is None:
                self.buf = self.g.clone()
            self.buf.mul_(MU).add_(r)
            d = w = self.buf
        y = self.retr(p, -LR * d)
        w.copy_(self.transp(p, y, w))
        p.copy_(y)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_riemannian_step.py measures on the GPU; none is visible")
    from hypad_amd import optim
    from hypad_amd.hyperspace import gmath
    from hypad_amd.hyperspace import hyrnn_nets as hn

    result = {"inner": args.inner, "samples": args.samples, "warmup": args.warmup, "lr": LR, "shapes": {}}
    for rows, D in SHAPES:
        g = torch.Generator().manual_seed(0)
        starts = {"ball": ball(g, (rows, D)), "sphere": torch.nn.functional.normalize(torch.randn(rows, D, generator=g).double(), dim=-1).float()}
        grad = torch.randn(rows, D, generator=g).cuda()
        shape_entry = {}
        print(f"({rows}, {D})")
        for man in ("ball", "sphere"):
            for rule in ("adam", "sgd"):
                prm = hn.ManifoldParameter(starts[man].cuda(), manifold=hn.PoincareBall() if man == "ball" else hn.Sphere())
                prm.grad = grad
                if rule == "adam":
                    opt = optim.RiemannianAdam([prm], lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD, manifold_rows=True)
                else:
                    opt = optim.RiemannianSGD([prm], lr=LR, momentum=MU, weight_decay=WD)
                comp = Composed(gmath, man, rule, starts[man].cuda(), grad)
                opt.step()
                comp.step()
                d = float((prm.detach() - comp.p).abs().max())                 # the first step of each: fp32 parameters, |p| <= 1
                tensors = 3 if rule == "adam" else 2                            # the parameter and its state: read and written; the gradient: read
                nbytes = 4 * rows * D * (2 * tensors + 1)
                for _ in range(args.warmup):
                    sample(opt.step, args.inner), sample(comp.step, args.inner)
                tf, tc = [], []
                for _ in range(args.samples):
                    tf.append(sample(opt.step, args.inner))
                    tc.append(sample(comp.step, args.inner))
                mf, mc = statistics.median(tf), statistics.median(tc)
                gbs = nbytes / mf * 1e-3
                name = f"{man}/{rule}"
                print(f"  {name:12s} fused {mf:9.1f} us ({min(tf):.1f} .. {max(tf):.1f})  {gbs:7.1f} GB/s   composed {mc:9.1f} us "
                      f"({min(tc):.1f} .. {max(tc):.1f})   composed / fused {mc / mf:.2f}   first step: max |fused - composed| {d:.1e}", flush=True)
                shape_entry[name] = {"fused": mf, "fused_min": min(tf), "fused_max": max(tf), "composed": mc, "composed_min": min(tc),
                                     "composed_max": max(tc), "algorithmic_bytes": nbytes, "fused_gb_per_s": gbs, "first_step_max_abs_diff": d}
        result["shapes"][f"{rows}x{D}"] = shape_entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
