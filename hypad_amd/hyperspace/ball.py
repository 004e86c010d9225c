"""The row-wise ball functions at any negative curvature k = -c: the autograd plumbing behind the methods of
``hyrnn_nets.PoincareBall(c)`` (docs/history/curvature.md).

At c == 1 a method is the ``gmath`` function of its name, bit for bit.  At any other finite c > 0 it runs the ``hypad_ball_<name>_*`` entry
points (csrc/tangent.hip), which take c by value: with s = sqrt(c) the kernels scale the operands by their power of s after the load and
the result before the store, around the same per-row fp64 maps the k = -1 kernels run.  Operand rules and refusals are those of the
``gmath`` function of the same name and come before any device call; what ``gmath`` hands to its kernels as a one-row broadcast (the bias
of mobius_add, the one-row w of mobius_pointwise_mul) is expanded here instead, which leaves the sum of that gradient to autograd.
The autograd functions are ``gmath``'s -- ``_RowMap``, ``_TimeRowMap``, ``_RowScalar`` and ``_Projection`` with c in place of None
(docs/history/row_plumbing.md); this module holds the operand rules alone.

The matmul forms -- dist_matmul, weighted_midpoint, weighted_midpoint_bmm, hyperbolic_attention -- run the k = -1 kernels of csrc/dist.hip,
midpoint.hip and attention.hip with c in their fp64 stages (``hypad_ball_dist_matmul_*`` and the like, docs/history/curvature_matmul.md):
the reference's formulas at k = -c, whose floors sit on the unscaled quantities.  Their operand rules and their autograd functions are
``gmath``'s own code: those functions take c as an optional last argument and then call the ``hypad_ball_*`` entry of their name.
"""
import math

import torch

from .. import _C
from . import gmath


def dist_matmul(c, x, y):
    return gmath._dist_matmul(x, y, lambda x3, y3: gmath._DistMatmul.apply(x3, y3, c))


def weighted_midpoint_bmm(c, xs, weights, lincomb):
    return gmath._weighted_midpoint_bmm(xs, weights, lincomb, lambda x3, w3, flags: gmath._WeightedMidpointBmm.apply(x3, w3, flags, c))


def weighted_midpoint(c, xs, weights, reducedim, dim, keepdim, lincomb, posweight, coadd):
    return gmath._weighted_midpoint(xs, weights, reducedim, dim, keepdim, lincomb, posweight, coadd,
                                    lambda x3, w2, flags: gmath._WeightedMidpoint.apply(x3, w2, flags, c))


def hyperbolic_attention(c, q, keys, values, beta, bias):
    return gmath._hyperbolic_attention(q, keys, values, beta, bias, lambda q3, k3, v3, b, bt: gmath._HyperbolicAttention.apply(q3, k3, v3, b, bt, c))


def curvature(ball, what):
    """c of ``ball`` as a host float: read from the CPU tensor the class stores, so nothing waits for the device.  Refused: a c that is
    not finite and positive, one that requires grad (learnable curvature is not implemented), one that lives on a device."""
    c = ball.c
    if isinstance(c, torch.Tensor):
        if c.requires_grad:
            raise NotImplementedError(f"PoincareBall.{what}: a curvature that requires grad is not implemented; supported: a fixed c > 0")
        if c.numel() != 1 or c.device.type != "cpu":
            raise NotImplementedError(f"PoincareBall.{what}: c {tuple(c.shape)} on {c.device} is not implemented; supported: one value on the host")
        c = c.item()
    c = float(c)
    if not (c > 0.0) or not math.isfinite(c):
        raise NotImplementedError(f"PoincareBall.{what}: c = {c} is not implemented; supported: a finite c > 0 (k = -c < 0)")
    return c


_ROWS_SUPPORTED = "supported: dim = -1 (the last dimension), floating operands, which are cast to fp32, rows of 1 to 256 elements"


def cast_rows(what, dim, **ops):
    """The operands of the functions that cast (project, expmap0, logmap0, mobius_add, mobius_pointwise_mul, mobius_scalar_mul): fp32,
    the last dimension only, 1 to 256 elements a row.  The methods ask this at c == 1 too, where gmath's own functions leave the
    width to the entry point."""
    ts = list(ops.values())
    desc = ", ".join(f"{n} {tuple(t.shape)} {t.dtype}" for n, t in ops.items())
    if any(t.dim() < 1 or not t.is_floating_point() or t.shape[-1] != ts[0].shape[-1] for t in ts) or not 1 <= ts[0].shape[-1] <= 256:
        raise NotImplementedError(f"{what}: {desc} is not implemented; {_ROWS_SUPPORTED}")
    nd = max(t.dim() for t in ts)
    if dim != -1 and dim != nd - 1:
        raise NotImplementedError(f"{what}: dim = {dim} on {desc} is not implemented; {_ROWS_SUPPORTED}")
    return [t.to(torch.float32) for t in ts]


def unary(name, c, x, dim):
    (x,) = cast_rows(name, dim, x=x)
    return gmath._RowMap.apply(name, c, x)


def mobius_add(c, x, y, dim):
    x, y = cast_rows("mobius_add", dim, x=x, y=y)
    try:
        x, y = torch.broadcast_tensors(x, y)
    except RuntimeError:
        raise _C.HypadError(f"mobius_add: x {tuple(x.shape)} and y {tuple(y.shape)} do not broadcast against each other") from None
    return gmath._RowMap.apply("mobius_add", c, x, y)


def mobius_pointwise_mul(c, w, x, dim):
    if x.dim() < 1 or w.dim() < 1 or w.shape[-1] != x.shape[-1] or (w.shape != x.shape and w.numel() != w.shape[-1]):
        raise NotImplementedError(f"mobius_pointwise_mul: w {tuple(w.shape)} against x {tuple(x.shape)} is not implemented; supported: w of the "
                                  f"shape of x or one row of it; {_ROWS_SUPPORTED}")
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"mobius_pointwise_mul: dim = {dim} is not implemented; {_ROWS_SUPPORTED}")
    w, x = cast_rows("mobius_pointwise_mul", -1, w=w, x=x)
    return gmath._RowMap.apply("mobius_pointwise_mul", c, w.reshape(-1).expand(x.shape) if w.shape != x.shape else w, x)


def mobius_scalar_mul(c, r, x, dim):
    (x,) = cast_rows("mobius_scalar_mul", dim, x=x)
    if not isinstance(r, torch.Tensor):
        r = torch.tensor(float(r), dtype=torch.float32, device=x.device)
    if not r.is_floating_point() or (r.numel() != 1 and tuple(r.shape) != tuple(x.shape[:-1]) + (1,)):
        raise NotImplementedError(f"mobius_scalar_mul: r {tuple(r.shape)} {r.dtype} against x {tuple(x.shape)} is not implemented; supported: r of "
                                  f"one element or of shape x.shape[:-1] + (1,); {_ROWS_SUPPORTED}")
    return gmath._TimeRowMap.apply("mobius_scalar_mul", c, r.to(torch.float32), x)


def rows(name, c, dim, **ops):
    return gmath._RowMap.apply(name, c, *gmath._tangent_operands(name, None, dim, **ops))


def timed(name, c, t, dim, **ops):
    x, y = gmath._tangent_operands(name, None, dim, **ops)
    t, x = gmath._time_operand(name, t, x)
    return gmath._TimeRowMap.apply(name, c, t, x, y)


def per_row(name, c, keepdim, dim, **ops):
    return gmath._per_row(gmath._RowScalar.apply(name, c, *gmath._tangent_operands(name, None, dim, **ops)), keepdim)


def dist(c, x, y, keepdim, dim):
    gmath._dist_refusals("dist", x, None, dim)
    if y.shape != x.shape or y.dtype != torch.float32:
        raise NotImplementedError(f"dist: y {tuple(y.shape)} {y.dtype} against x {tuple(x.shape)} is not implemented; {gmath._DIST_SUPPORTED}")
    return gmath._per_row(gmath._RowScalar.apply("dist", c, x, y), keepdim)


def dist0(c, x, keepdim, dim):
    gmath._dist_refusals("dist0", x, None, dim)
    return gmath._per_row(gmath._RowScalar.apply("dist0", c, x), keepdim)


def projection(name, c, x, dim, grow):
    gmath._projection_refusals(name, x, None, dim, grow)
    return gmath._Projection.apply(name, c, x, grow)
