"""Poincare-ball ops (k = -1) on the GPU, with autograd.

Drop-in for the geoopt functions the reference's hot path reaches through
``geoopt.manifolds.stereographic.math`` (vendored at /root/reference/math_.py): expmap0 (:1132-1136),
logmap0 (:1267-1270), mobius_add (:536-555), project (:340-352), plus the inline row-wise distance of
train.py:226-230 and the hyperbolic loss of train.py:232.  Each is one HIP kernel forward and one backward.
dist2plane (:1599-1666) is the function behind hyrnn_nets.MobiusDist2Hyperplane: one HIP launch forward, a HIP backward.
mobius_pointwise_mul (:1328-1371) is the gate product of the Moebius GRU (hyrnn_nets.mobius_gru_cell), here on its own.
"""
import torch

from .. import _C

_K_MSG = "only curvature k = -1 is implemented (the only value HypAD uses: hyperspace/hyrnn_nets.py:20,166)"


def _check_k(k):
    if k is not None and abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(_K_MSG)


def _rows(t):
    t = t.to(torch.float32).contiguous()
    _C.require_cuda(t)
    return t, t.reshape(-1, t.shape[-1])


def _rows_width(t):
    """(rows, width) of t taken as rows of its last dimension, from the shape alone."""
    rows = 1
    for n in t.shape[:-1]:
        rows *= n
    return rows, t.shape[-1]


def _same_shape(what, u, v):
    """The row kernels take one (rows, dim) for both operands and broadcast nothing: refused here, before any device tensor is asked
    for (the entry point would read v with u's sizes)."""
    if u.dim() < 1 or u.shape != v.shape:
        raise _C.HypadError(f"{what}: u {tuple(u.shape)} and v {tuple(v.shape)} must have the same shape (nothing is broadcast)")


class _Unary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, fwd, bwd):
        x, x2 = _rows(x)
        out = torch.empty_like(x2)
        _C.check(getattr(_C.lib, fwd)(_C.ptr(x2), _C.ptr(out), x2.shape[0], x2.shape[1], _C.stream()), fwd)
        ctx.save_for_backward(x2)
        ctx.bwd, ctx.shape = bwd, x.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        (x2,) = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gx = torch.empty_like(x2)
        _C.check(getattr(_C.lib, ctx.bwd)(_C.ptr(x2), _C.ptr(go2), _C.ptr(gx), x2.shape[0], x2.shape[1], _C.stream()), ctx.bwd)
        return gx.view(ctx.shape), None, None


def expmap0(u, *, k=None, dim=-1):
    _check_k(k)
    return _Unary.apply(u, "hypad_expmap0_fwd", "hypad_expmap0_bwd")


def logmap0(y, *, k=None, dim=-1):
    _check_k(k)
    return _Unary.apply(y, "hypad_logmap0_fwd", "hypad_logmap0_bwd")


def project(x, *, k=None, dim=-1, eps=-1.0):
    _check_k(k)
    if eps >= 0:
        raise NotImplementedError("custom eps: the fused kernel uses the fp32 default 4e-3 (math_.py:343-347)")
    return _Unary.apply(x, "hypad_project_fwd", "hypad_project_bwd")


class _MobiusAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y):
        if x.dim() < 1 or y.dim() < 1 or _rows_width(y)[0] not in (1, _rows_width(x)[0]) or y.shape[-1] != x.shape[-1]:
            raise _C.HypadError(f"mobius_add: y {tuple(y.shape)} must have the rows of x {tuple(x.shape)} or a single (broadcast) row")
        x, x2 = _rows(x)
        y, y2 = _rows(y)
        yr = y2.shape[0]
        out = torch.empty_like(x2)
        _C.check(_C.lib.hypad_mobius_add_fwd(_C.ptr(x2), _C.ptr(y2), _C.ptr(out), x2.shape[0], x2.shape[1], yr, _C.stream()))
        ctx.save_for_backward(x2, y2)
        ctx.xs, ctx.ys = x.shape, y.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, y2 = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gx, gy = torch.empty_like(x2), torch.empty_like(x2)
        _C.check(_C.lib.hypad_mobius_add_bwd(_C.ptr(x2), _C.ptr(y2), _C.ptr(go2), _C.ptr(gx), _C.ptr(gy), x2.shape[0],
                                             x2.shape[1], y2.shape[0], _C.stream()))
        if y2.shape[0] == 1 and x2.shape[0] != 1:
            red = torch.empty(1, x2.shape[1], device=x2.device, dtype=torch.float32)
            _C.check(_C.lib.hypad_column_sum(_C.ptr(gy), _C.ptr(red), x2.shape[0], x2.shape[1], _C.stream()))
            gy = red
        return gx.view(ctx.xs), gy.view(ctx.ys)


def mobius_add(x, y, *, k=None, dim=-1):
    _check_k(k)
    if x.dim() < 1 or y.dim() < 1 or y.shape[-1] != x.shape[-1]:
        raise _C.HypadError(f"mobius_add: x {tuple(x.shape)} and y {tuple(y.shape)} differ in their last dimension")
    if y.dim() == x.dim() and y.shape != x.shape:
        y = y.expand_as(x)
    if y.dim() < x.dim():
        y = y.reshape(1, -1)
    return _MobiusAdd.apply(x, y)


class _MobiusPointwiseMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, x):
        x, x2 = _rows(x)
        w, w2 = _rows(w)
        out = torch.empty_like(x2)
        _C.check(_C.lib.hypad_mobius_pointwise_mul_fwd(_C.ptr(w2), _C.ptr(x2), _C.ptr(out), x2.shape[0], x2.shape[1], w2.shape[0], _C.stream()),
                 "mobius_pointwise_mul_fwd")
        ctx.save_for_backward(w2, x2)
        ctx.ws, ctx.xs = w.shape, x.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        w2, x2 = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gw, gx = torch.empty_like(x2), torch.empty_like(x2)
        _C.check(_C.lib.hypad_mobius_pointwise_mul_bwd(_C.ptr(w2), _C.ptr(x2), _C.ptr(go2), _C.ptr(gw), _C.ptr(gx), x2.shape[0], x2.shape[1],
                                                       w2.shape[0], _C.stream()), "mobius_pointwise_mul_bwd")
        if w2.shape[0] == 1 and x2.shape[0] != 1:
            red = torch.empty(1, x2.shape[1], device=x2.device, dtype=torch.float32)
            _C.check(_C.lib.hypad_column_sum(_C.ptr(gw), _C.ptr(red), x2.shape[0], x2.shape[1], _C.stream()))
            gw = red
        return gw.view(ctx.ws), gx.view(ctx.xs)


_PMUL_SUPPORTED = "supported: k = -1, dim = -1, fp32, w of the shape of x or one row of it, rows of at most 256 elements"


def mobius_pointwise_mul(w, x, *, k=None, dim=-1):
    """diag(w) (x) x for ball-valued rows of x (math_.py:1328-1371) at k = -1: one HIP launch forward and one backward, first-order
    differentiable in w and x.  w has the shape of x, or is a single row broadcast over the rows of x."""
    if k is not None and abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(f"mobius_pointwise_mul: curvature k = {float(k)} is not implemented; {_PMUL_SUPPORTED}")
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"mobius_pointwise_mul: dim = {dim} is not implemented; {_PMUL_SUPPORTED}")
    one_row = w.dim() >= 1 and w.numel() == w.shape[-1]
    if x.dim() < 1 or w.dim() < 1 or w.shape[-1] != x.shape[-1] or (w.shape != x.shape and not one_row):
        raise NotImplementedError(f"mobius_pointwise_mul: w {tuple(w.shape)} against x {tuple(x.shape)} is not implemented; {_PMUL_SUPPORTED}")
    if x.shape[-1] > 256:
        raise NotImplementedError(f"mobius_pointwise_mul: rows of {x.shape[-1]} elements are not implemented; {_PMUL_SUPPORTED}")
    return _MobiusPointwiseMul.apply(w.reshape(1, -1) if one_row and w.shape != x.shape else w, x)


def mobius_fn_apply(fn, x, *args, k=None, dim=-1, **kwargs):
    """expmap0(fn(logmap0(x)))  (math_.py:1431-1469): the two maps are the HIP kernels above (first-order gradients, as theirs);
    ``fn`` is the caller's own function of the tangent vector.  Inside mobius_linear, tanh and relu run fused in the layer's
    kernels instead (hyrnn_nets.mobius_linear)."""
    _check_k(k)
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError("mobius_fn_apply: only the last dimension (dim = -1) is implemented")
    return expmap0(fn(logmap0(x), *args, **kwargs))


def mobius_matvec(m, x, *, k=None, dim=-1):
    """math_.py:1308-1323: see hyrnn_nets.mobius_matvec (one HIP launch, differentiable in m and x)."""
    from .hyrnn_nets import mobius_matvec as _matvec
    return _matvec(m, x, k=-1.0 if k is None else k, dim=dim)


class _Dist2Plane(torch.autograd.Function):
    """hypad_dist2plane_*: x (..., K) against p, a (N, K) -> (..., N), times exp(log_scale) (N) inside the kernel where given.
    Nothing but the operands is saved: the backward recomputes the two products."""

    @staticmethod
    def forward(ctx, x, p, a, log_scale, flags):
        if (p.dim() != 2 or a.shape != p.shape or x.dim() < 1 or x.shape[-1] != p.shape[1]
                or (log_scale is not None and tuple(log_scale.shape) != (p.shape[0],))):
            raise _C.HypadError(f"dist2plane: x {tuple(x.shape)} against p {tuple(p.shape)}, a {tuple(a.shape)}"
                                + ("" if log_scale is None else f" and scale {tuple(log_scale.shape)}")
                                + ": p and a must be (out_features, in_features), x (..., in_features), scale (out_features,)")
        x, x2 = _rows(x)
        p = _C.require_cuda(p.contiguous(), "p")
        a = _C.require_cuda(a.contiguous(), "a")
        ls = None if log_scale is None else _C.require_cuda(log_scale.contiguous(), "log_scale")
        rows, k, n = x2.shape[0], x2.shape[1], p.shape[0]
        out = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_dist2plane_fwd(_C.ptr(x2), _C.ptr(p), _C.ptr(a), _C.ptr(ls), _C.ptr(out), rows, k, n, flags, _C.stream()),
                 "dist2plane_fwd")
        ctx.save_for_backward(x2, p, a, *(() if ls is None else (ls,)))
        ctx.xshape, ctx.flags = x.shape, flags
        return out.view(*x.shape[:-1], n)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, p, a, *rest = ctx.saved_tensors
        ls = rest[0] if rest else None
        rows, k, n = x2.shape[0], x2.shape[1], p.shape[0]
        go2 = go.to(torch.float32).contiguous().reshape(rows, n)
        need = ctx.needs_input_grad
        gx = torch.empty_like(x2) if need[0] else None
        gp = torch.empty_like(p) if need[1] else None
        ga = torch.empty_like(a) if need[2] else None
        gs = torch.empty_like(ls) if ls is not None and need[3] else None
        nbytes = _C.lib.hypad_dist2plane_workspace_bytes(rows, k, n)
        ws = torch.empty(max(nbytes // 4, 1), device=x2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_dist2plane_bwd(_C.ptr(x2), _C.ptr(p), _C.ptr(a), _C.ptr(ls), None, _C.ptr(go2), _C.ptr(gx), _C.ptr(gp),
                                             _C.ptr(ga), _C.ptr(gs), _C.ptr(ws), nbytes, rows, k, n, ctx.flags, _C.stream()), "dist2plane_bwd")
        return None if gx is None else gx.view(ctx.xshape), gp, ga, gs, None


_D2P_SUPPORTED = ("supported: k = -1, dim = -1, fp32, x of shape (..., 1, K) against 2-D p and a of shape (N, K) (the layer's calling "
                  "pattern, hyperspace/hyrnn_nets.py:233-236), K <= 256")


def dist2plane(x, p, a, *, k=None, keepdim=False, signed=False, scaled=False, dim=-1):
    """Geodesic distance of x to the hyperplanes through p with normals a (math_.py:1599-1666) at k = -1, for the layer's calling
    pattern: x (..., 1, K) against p, a (N, K) -> (..., N), or (..., N, 1) with keepdim.  One HIP launch forward; first-order
    differentiable in x, p and a."""
    if k is not None and abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(f"dist2plane: curvature k = {float(k)} is not implemented; {_D2P_SUPPORTED}")
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"dist2plane: dim = {dim} is not implemented; {_D2P_SUPPORTED}")
    if (p.dim() != 2 or a.shape != p.shape or x.dim() < 2 or x.shape[-2] != 1 or x.shape[-1] != p.shape[-1]):
        raise NotImplementedError(f"dist2plane: x {tuple(x.shape)} against p {tuple(p.shape)} and a {tuple(a.shape)} is not implemented; "
                                  f"{_D2P_SUPPORTED}")
    if p.shape[-1] > 256:
        raise NotImplementedError(f"dist2plane: K = {p.shape[-1]} is not implemented; {_D2P_SUPPORTED}")
    flags = (_C.D2P_SIGNED if signed else 0) | (_C.D2P_SCALED if scaled else 0)
    out = _Dist2Plane.apply(x.squeeze(-2), p, a, None, flags)
    return out.unsqueeze(-1) if keepdim else out


class _RowDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v):
        _same_shape("poincare_rowdist", u, v)
        u, u2 = _rows(u)
        v, v2 = _rows(v)
        out = torch.empty(u2.shape[0], device=u2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_poincare_rowdist_fwd(_C.ptr(u2), _C.ptr(v2), _C.ptr(out), u2.shape[0], u2.shape[1], _C.stream()))
        ctx.save_for_backward(u2, v2)
        ctx.us, ctx.vs = u.shape, v.shape
        return out.view(u.shape[:-1])

    @staticmethod
    @_C.first_order_only
    def backward(ctx, gd):
        u2, v2 = ctx.saved_tensors
        gd = gd.to(torch.float32).contiguous().reshape(-1)
        gu, gv = torch.empty_like(u2), torch.empty_like(v2)
        _C.check(_C.lib.hypad_poincare_rowdist_bwd(_C.ptr(u2), _C.ptr(v2), _C.ptr(gd), _C.ptr(gu), _C.ptr(gv), u2.shape[0],
                                                   u2.shape[1], _C.stream()))
        return gu.view(ctx.us), gv.view(ctx.vs)


def poincare_rowdist(u, v):
    """acosh(1 + 2|u-v|^2 / ((1-|u|^2)(1-|v|^2)) + 1e-7) per row (train.py:226-230)."""
    return _RowDist.apply(u, v)


class _HyperLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, batch):
        _same_shape("hyperbolic_loss", u, v)
        u, u2 = _rows(u)
        v, v2 = _rows(v)
        out = torch.empty(1, device=u2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_hyper_loss_fwd(_C.ptr(u2), _C.ptr(v2), _C.ptr(out), u2.shape[0], u2.shape[1], int(batch), _C.stream()))
        ctx.save_for_backward(u2, v2)
        ctx.us, ctx.vs, ctx.batch = u.shape, v.shape, int(batch)
        return out.view(())

    @staticmethod
    @_C.first_order_only
    def backward(ctx, g):
        u2, v2 = ctx.saved_tensors
        gu, gv = torch.empty_like(u2), torch.empty_like(v2)
        # The incoming gradient stays on the device (float(g) would make the host wait for the stream on every backward, and cannot be
        # captured): g / batch per row, the same fp32 division hypad_hyper_loss_bwd does on the host, into the row-distance backward --
        # the same kernel with gd[r] in place of its scalar.  (Both operands are tensors: torch divides by a host scalar by
        # multiplying with its reciprocal, which is not the same bits.)
        rows = u2.shape[0]
        if rows == 0:
            return gu.view(ctx.us), gv.view(ctx.vs), None
        gd = g.to(torch.float32).reshape(1).expand(rows) / torch.full((rows,), float(ctx.batch), device=u2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_poincare_rowdist_bwd(_C.ptr(u2), _C.ptr(v2), _C.ptr(gd), _C.ptr(gu), _C.ptr(gv), rows, u2.shape[1], _C.stream()))
        return gu.view(ctx.us), gv.view(ctx.vs), None


def hyperbolic_loss(u, v, batch_size):
    """torch.div(torch.sum(dist), batch_size)  (train.py:232)."""
    return _HyperLoss.apply(u, v, batch_size)
