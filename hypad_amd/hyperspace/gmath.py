"""Poincare-ball ops (k = -1) on the GPU, with autograd.

Drop-in for the geoopt functions the reference's hot path reaches through
``geoopt.manifolds.stereographic.math`` (vendored at /root/reference/math_.py): expmap0 (:1132-1136),
logmap0 (:1267-1270), mobius_add (:536-555), project (:340-352), plus the inline row-wise distance of
train.py:226-230 and the hyperbolic loss of train.py:232.  Each is one HIP kernel forward and one backward.
dist2plane (:1599-1666) is the function behind hyrnn_nets.MobiusDist2Hyperplane: one HIP launch forward, a HIP backward.
mobius_pointwise_mul (:1328-1371) is the gate product of the Moebius GRU (hyrnn_nets.mobius_gru_cell), here on its own.
weighted_midpoint (:1953-2087) and weighted_midpoint_bmm (:2090-2122) turn many ball points into one -- pooling over dimensions of one
tensor, and weights (..., N, M) against xs (..., M, D) for attention and aggregation; mobius_scalar_mul (:788-858) is their lincomb step
and an op of its own.  HIP kernels forward and backward (docs/history/weighted_midpoint.md).
dist_matmul (:905-947) is the geodesic distance of every point of x from every point of y -- the score of hyperbolic attention --, dist
(:861-902) and dist0 (:950-975) its row forms: HIP kernels forward and backward (docs/history/geodesic_distance.md).
hyperbolic_attention is dist_matmul, a softmax and weighted_midpoint_bmm as one function whose kernels keep no (N, M) tensor
(docs/history/hyperbolic_attention.md).
expmap (:1052-1102), logmap (:1188-1230), geodesic (:978-1049), gyration (:592-675), parallel_transport (:1669-1746),
parallel_transport0 (:1749-1779) and parallel_transport0back (:1782-1813) are the tangent maps at an arbitrary point of the ball: one
HIP launch forward and one backward each, operands broadcast against each other (docs/history/tangent_maps.md).
mobius_sub (:558-589), mobius_coadd (:678-744), mobius_cosub (:747-779) and geodesic_unit (:1139-1185) are the rest of the gyrogroup;
lambda_x (:355-383), inner (:386-430), norm (:433-472) and egrad2rgrad (:1816-1845) the Riemannian metric -- with expmap the pieces of a
hand-written Riemannian update --; sproj (:1848-1874) and inv_sproj (:1877-1905) move between the ball and the hyperboloid: one HIP launch
forward and one backward each.  antipode (:1908-1950), mobius_fn_apply_chain (:1374-1428) and mobiusify (:1472-1498) need no kernel of
their own (docs/history/gyro_ops.md).
dist2plane_matmul (:2125-2159) is the batched hyperplane read-out in the operand layout of dist_matmul -- the reference's own formula,
which is not 2 dist2plane(...) --: one HIP launch forward, two fused launches backward (docs/history/dist2plane_matmul.md).  With it every
public function of math_.py has its counterpart here.
"""
import torch

from .. import _C

_K_MSG = "only curvature k = -1 is implemented (the only value HypAD uses: hyperspace/hyrnn_nets.py:20,166)"
_ROW_SUPPORTED = "supported: k = -1, dim = -1 (the last dimension), floating operands, which are cast to fp32 (the result is fp32)"


def _check_k(k):
    if k is not None and abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(_K_MSG)


def _refuse_k(what, k, supported):
    """The refusal of any curvature but k = -1 (None: the default), in the words of the functions after the first generation."""
    if k is not None and abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(f"{what}: curvature k = {float(k)} is not implemented; {supported}")


def _check_last_dim(what, x, dim):
    """The row kernels work along the last dimension alone: any other ``dim`` is refused, not ignored."""
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"{what}: dim = {dim} on an operand {tuple(x.shape)} is not implemented; {_ROW_SUPPORTED}")


def _rows(t):
    t = t.to(torch.float32).contiguous()
    _C.require_cuda(t)
    return t, t.reshape(-1, t.shape[-1])


def _launch(rows, entry, *args):
    """The entry point ``entry`` over ``rows`` rows.  Without rows nothing is called: there is nothing to launch, and the data pointer
    of an empty tensor is null, which the entry points refuse."""
    if rows:
        _C.check(getattr(_C.lib, entry)(*args), entry)


def _column_sum(g):
    """(rows, n) -> (1, n): the rows' contributions to the gradient of a one-row operand, added in a fixed order; zeros over no rows."""
    rows, n = g.shape
    if rows == 0:
        return torch.zeros(1, n, device=g.device, dtype=torch.float32)
    red = torch.empty(1, n, device=g.device, dtype=torch.float32)
    _C.check(_C.lib.hypad_column_sum(_C.ptr(g), _C.ptr(red), rows, n, _C.stream()), "hypad_column_sum")
    return red


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
        _launch(x2.shape[0], fwd, _C.ptr(x2), _C.ptr(out), x2.shape[0], x2.shape[1], _C.stream())
        ctx.save_for_backward(x2)
        ctx.bwd, ctx.shape = bwd, x.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        (x2,) = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gx = torch.empty_like(x2)
        _launch(x2.shape[0], ctx.bwd, _C.ptr(x2), _C.ptr(go2), _C.ptr(gx), x2.shape[0], x2.shape[1], _C.stream())
        return gx.view(ctx.shape), None, None


def expmap0(u, *, k=None, dim=-1):
    """tanh(|u|) u / |u| along the last dimension (math_.py:1132-1136) at k = -1.  A floating operand of any dtype is cast to fp32 and the
    result is fp32; any other ``dim`` is refused."""
    _check_k(k)
    _check_last_dim("expmap0", u, dim)
    return _Unary.apply(u, "hypad_expmap0_fwd", "hypad_expmap0_bwd")


def logmap0(y, *, k=None, dim=-1):
    """artanh(|y|) y / |y| along the last dimension (math_.py:1267-1270) at k = -1.  A floating operand of any dtype is cast to fp32 and
    the result is fp32; any other ``dim`` is refused."""
    _check_k(k)
    _check_last_dim("logmap0", y, dim)
    return _Unary.apply(y, "hypad_logmap0_fwd", "hypad_logmap0_bwd")


def project(x, *, k=None, dim=-1, eps=-1.0):
    """Rows beyond the norm 1 - 4e-3 scaled back onto it (math_.py:340-352) at k = -1.  A floating operand of any dtype is cast to fp32
    and the result is fp32 (with the fp32 eps); any other ``dim`` is refused."""
    _check_k(k)
    _check_last_dim("project", x, dim)
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
        _launch(x2.shape[0], "hypad_mobius_add_fwd", _C.ptr(x2), _C.ptr(y2), _C.ptr(out), x2.shape[0], x2.shape[1], yr, _C.stream())
        ctx.save_for_backward(x2, y2)
        ctx.xs, ctx.ys = x.shape, y.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, y2 = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gx, gy = torch.empty_like(x2), torch.empty_like(x2)
        _launch(x2.shape[0], "hypad_mobius_add_bwd", _C.ptr(x2), _C.ptr(y2), _C.ptr(go2), _C.ptr(gx), _C.ptr(gy), x2.shape[0], x2.shape[1],
                y2.shape[0], _C.stream())
        if y2.shape[0] == 1 and x2.shape[0] != 1:
            gy = _column_sum(gy)
        return gx.view(ctx.xs), gy.view(ctx.ys)


def mobius_add(x, y, *, k=None, dim=-1):
    """x (+) y along the last dimension (math_.py:536-555) at k = -1: one HIP launch forward and one backward.  The leading dimensions
    of x and y broadcast against each other by torch's rules.  A y of a single row and fewer dimensions than x -- the bias of a layer --
    is broadcast inside the kernel and its gradient summed there; every other broadcast operand is expanded and materialised, which
    leaves the sum of its gradient to autograd (the expand's backward).  Floating operands of any dtype are cast to fp32 and the result
    is fp32; any other ``dim`` is refused."""
    _check_k(k)
    if x.dim() < 1 or y.dim() < 1 or y.shape[-1] != x.shape[-1]:
        raise _C.HypadError(f"mobius_add: x {tuple(x.shape)} and y {tuple(y.shape)} differ in their last dimension")
    _check_last_dim("mobius_add", x if x.dim() >= y.dim() else y, dim)
    if y.dim() < x.dim() and y.numel() == y.shape[-1]:
        return _MobiusAdd.apply(x, y.reshape(1, -1))
    if y.shape != x.shape:
        try:
            shape = torch.broadcast_shapes(tuple(x.shape), tuple(y.shape))
        except RuntimeError:
            raise _C.HypadError(f"mobius_add: x {tuple(x.shape)} and y {tuple(y.shape)} do not broadcast against each other") from None
        x, y = x.expand(shape), y.expand(shape)
    return _MobiusAdd.apply(x, y)


class _MobiusPointwiseMul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, x):
        x, x2 = _rows(x)
        w, w2 = _rows(w)
        out = torch.empty_like(x2)
        _launch(x2.shape[0], "hypad_mobius_pointwise_mul_fwd", _C.ptr(w2), _C.ptr(x2), _C.ptr(out), x2.shape[0], x2.shape[1], w2.shape[0],
                _C.stream())
        ctx.save_for_backward(w2, x2)
        ctx.ws, ctx.xs = w.shape, x.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        w2, x2 = ctx.saved_tensors
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gw, gx = torch.empty_like(x2), torch.empty_like(x2)
        _launch(x2.shape[0], "hypad_mobius_pointwise_mul_bwd", _C.ptr(w2), _C.ptr(x2), _C.ptr(go2), _C.ptr(gw), _C.ptr(gx), x2.shape[0],
                x2.shape[1], w2.shape[0], _C.stream())
        if w2.shape[0] == 1 and x2.shape[0] != 1:
            gw = _column_sum(gw)
        return gw.view(ctx.ws), gx.view(ctx.xs)


_PMUL_SUPPORTED = "supported: k = -1, dim = -1, fp32, w of the shape of x or one row of it, rows of at most 256 elements"


def mobius_pointwise_mul(w, x, *, k=None, dim=-1):
    """diag(w) (x) x for ball-valued rows of x (math_.py:1328-1371) at k = -1: one HIP launch forward and one backward, first-order
    differentiable in w and x.  w has the shape of x, or is a single row broadcast over the rows of x.  Floating operands of any dtype
    are cast to fp32 and the result is fp32."""
    _refuse_k("mobius_pointwise_mul", k, _PMUL_SUPPORTED)
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"mobius_pointwise_mul: dim = {dim} is not implemented; {_PMUL_SUPPORTED}")
    one_row = w.dim() >= 1 and w.numel() == w.shape[-1]
    if x.dim() < 1 or w.dim() < 1 or w.shape[-1] != x.shape[-1] or (w.shape != x.shape and not one_row):
        raise NotImplementedError(f"mobius_pointwise_mul: w {tuple(w.shape)} against x {tuple(x.shape)} is not implemented; {_PMUL_SUPPORTED}")
    if x.shape[-1] > 256:
        raise NotImplementedError(f"mobius_pointwise_mul: rows of {x.shape[-1]} elements are not implemented; {_PMUL_SUPPORTED}")
    return _MobiusPointwiseMul.apply(w.reshape(1, -1) if one_row and w.shape != x.shape else w, x)


class _MobiusScalarMul(torch.autograd.Function):
    """hypad_mobius_scalar_mul_*: r of one element, or of one element per row of x."""

    @staticmethod
    def forward(ctx, r, x):
        x, x2 = _rows(x)
        r1 = _C.require_cuda(r.to(torch.float32).contiguous().reshape(-1), "r")
        out = torch.empty_like(x2)
        _launch(x2.shape[0], "hypad_mobius_scalar_mul_fwd", _C.ptr(r1), _C.ptr(x2), _C.ptr(out), x2.shape[0], x2.shape[1], r1.shape[0],
                _C.stream())
        ctx.save_for_backward(r1, x2)
        ctx.rs, ctx.xs = r.shape, x.shape
        return out.view(x.shape)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        r1, x2 = ctx.saved_tensors
        rows = x2.shape[0]
        go2 = go.to(torch.float32).contiguous().reshape(x2.shape)
        gr = torch.empty(rows, device=x2.device, dtype=torch.float32) if ctx.needs_input_grad[0] else None
        gx = torch.empty_like(x2) if ctx.needs_input_grad[1] else None
        _launch(rows, "hypad_mobius_scalar_mul_bwd", _C.ptr(r1), _C.ptr(x2), _C.ptr(go2), _C.ptr(gr), _C.ptr(gx), rows, x2.shape[1], r1.shape[0],
                _C.stream())
        if gr is not None and r1.shape[0] == 1 and rows != 1:      # one r for every row: the rows' contributions, added in a fixed order
            gr = _column_sum(gr.view(rows, 1)).view(1)
        return None if gr is None else gr.view(ctx.rs), None if gx is None else gx.view(ctx.xs)


_SMUL_SUPPORTED = "supported: k = -1, dim = -1, fp32, r of one element or of shape x.shape[:-1] + (1,), rows of at most 256 elements"


def mobius_scalar_mul(r, x, *, k=None, dim=-1):
    """r (x) x = tanh(r artanh |x|) x / |x| for ball-valued rows of x (math_.py:788-858) at k = -1: one HIP launch forward and one
    backward, first-order differentiable in r and x.  r is a tensor of one element (or a number) or holds one value per row of x,
    shape x.shape[:-1] + (1,).  Floating operands of any dtype are cast to fp32 and the result is fp32."""
    _refuse_k("mobius_scalar_mul", k, _SMUL_SUPPORTED)
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"mobius_scalar_mul: dim = {dim} is not implemented; {_SMUL_SUPPORTED}")
    if x.dim() < 1 or x.shape[-1] > 256:
        raise NotImplementedError(f"mobius_scalar_mul: x {tuple(x.shape)} is not implemented; {_SMUL_SUPPORTED}")
    if not isinstance(r, torch.Tensor):
        r = torch.tensor(float(r), dtype=torch.float32, device=x.device)
    if r.numel() != 1 and tuple(r.shape) != tuple(x.shape[:-1]) + (1,):
        raise NotImplementedError(f"mobius_scalar_mul: r {tuple(r.shape)} against x {tuple(x.shape)} is not implemented; {_SMUL_SUPPORTED}")
    return _MobiusScalarMul.apply(r, x)


def _entry(name, c):
    """(the entry point ``hypad_<name>`` and nothing, or ``hypad_ball_<name>`` and c): the autograd functions of the matmul forms and
    of the row forms (``_row_call``) run at k = -1 (c None) and, for the methods of PoincareBall(c) (hyperspace/ball.py), at k = -c --
    the same argument list with c before the stream."""
    full = ("hypad_" if c is None else "hypad_ball_") + name
    return getattr(_C.lib, full), (() if c is None else (c,)), full


class _WeightedMidpointBmm(torch.autograd.Function):
    """hypad_weighted_midpoint_bmm_* (c given: hypad_ball_weighted_midpoint_bmm_*): xs (batch, M, D), weights (batch, N, M) -> (batch, N, D); saves the operands and
    [nom | den | alpha] (batch, N, D + 2)."""

    @staticmethod
    def forward(ctx, xs, weights, flags, c=None):
        xs = _C.require_cuda(xs.contiguous(), "xs")
        weights = _C.require_cuda(weights.contiguous(), "weights")
        batch, m, d = xs.shape
        n = weights.shape[1]
        out = torch.empty(batch, n, d, device=xs.device, dtype=torch.float32)
        train = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        saved = torch.empty(batch, n, d + 2, device=xs.device, dtype=torch.float32) if train else None
        fn, cv, name = _entry("weighted_midpoint_bmm_fwd", c)
        _C.check(fn(_C.ptr(xs), _C.ptr(weights), _C.ptr(out), _C.ptr(saved), batch, n, m, d, flags, *cv, _C.stream()), name)
        if train:
            ctx.save_for_backward(xs, weights, saved)
        ctx.flags, ctx.c = flags, c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        xs, weights, saved = ctx.saved_tensors
        batch, m, d = xs.shape
        n = weights.shape[1]
        go = go.to(torch.float32).contiguous()
        gx = torch.empty_like(xs) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(weights) if ctx.needs_input_grad[1] else None
        nbytes = _C.lib.hypad_weighted_midpoint_bmm_workspace_bytes(batch, n, m, d)
        ws = torch.empty(max(nbytes // 4, 1), device=xs.device, dtype=torch.float32)
        fn, cv, name = _entry("weighted_midpoint_bmm_bwd", ctx.c)
        _C.check(fn(_C.ptr(xs), _C.ptr(weights), _C.ptr(saved), _C.ptr(go), _C.ptr(gx), _C.ptr(gw), _C.ptr(ws), nbytes, batch, n, m, d, ctx.flags, *cv,
                    _C.stream()), name)
        return gx, gw, None, None


_BMM_SUPPORTED = ("supported: k = -1, fp32, xs (..., M, D) against weights (..., N, M) with the same leading batch dimensions on both, or "
                  "none on one of them, D <= 256")


def weighted_midpoint_bmm(xs, weights, k, lincomb=False):
    """The weighted Moebius gyromidpoint of the points xs (..., M, D) under every row of weights (..., N, M) -> (..., N, D)
    (math_.py:2090-2122) at k = -1: the aggregation step of a hyperbolic attention or graph layer.  One HIP launch forward on fp32
    MFMA; first-order differentiable in xs and weights.  Both operands carry the same leading batch dimensions, or one of them carries
    none: that operand is expanded over the batch and materialised on the host, and the sum of its gradient over the batch is left
    to autograd (the expand's backward)."""
    _refuse_k("weighted_midpoint_bmm", k, _BMM_SUPPORTED)
    return _weighted_midpoint_bmm(xs, weights, lincomb, _WeightedMidpointBmm.apply)


def _weighted_midpoint_bmm(xs, weights, lincomb, apply):
    """The operand rules of weighted_midpoint_bmm, then ``apply(xs3, weights3, flags)``: the k = -1 autograd function, or the one of
    PoincareBall(c) (hyperspace/ball.py)."""
    bx, bw = tuple(xs.shape[:-2]), tuple(weights.shape[:-2])
    if (xs.dim() < 2 or weights.dim() < 2 or weights.shape[-1] != xs.shape[-2] or (bx != bw and bx != () and bw != ())
            or xs.dtype != torch.float32 or weights.dtype != torch.float32):
        raise NotImplementedError(f"weighted_midpoint_bmm: xs {tuple(xs.shape)} {xs.dtype} against weights {tuple(weights.shape)} "
                                  f"{weights.dtype} is not implemented; {_BMM_SUPPORTED}")
    if xs.shape[-1] > 256:
        raise NotImplementedError(f"weighted_midpoint_bmm: D = {xs.shape[-1]} is not implemented; {_BMM_SUPPORTED}")
    lead = bx or bw
    if bx != lead:
        xs = xs.expand(*lead, *xs.shape[-2:])
    if bw != lead:
        weights = weights.expand(*lead, *weights.shape[-2:])
    out = apply(xs.reshape(-1, *xs.shape[-2:]), weights.reshape(-1, *weights.shape[-2:]), _C.MID_LINCOMB if lincomb else 0)
    return out.view(*lead, weights.shape[-2], xs.shape[-1])


class _WeightedMidpoint(torch.autograd.Function):
    """hypad_weighted_midpoint_* (c given: hypad_ball_weighted_midpoint_*): xs (M, R, D), weights (M, R), of one element, or None -> (R, D); saves the operands and
    [nom | den | alpha] (R, D + 2) in fp64."""

    @staticmethod
    def forward(ctx, xs, weights, flags, c=None):
        xs = _C.require_cuda(xs.contiguous(), "xs")
        m, r, d = xs.shape
        w = None if weights is None else _C.require_cuda(weights.contiguous().reshape(-1), "weights")
        wn = 0 if w is None else w.shape[0]
        out = torch.empty(r, d, device=xs.device, dtype=torch.float32)
        train = ctx.needs_input_grad[0] or (w is not None and ctx.needs_input_grad[1])
        saved = torch.empty(r, d + 2, device=xs.device, dtype=torch.float64) if train else None
        nbytes = _C.lib.hypad_weighted_midpoint_workspace_bytes(m, r, d)
        ws = torch.empty(max(nbytes // 4, 1), device=xs.device, dtype=torch.float32)
        fn, cv, name = _entry("weighted_midpoint_fwd", c)
        _C.check(fn(_C.ptr(xs), _C.ptr(w), wn, _C.ptr(out), _C.ptr(saved), _C.ptr(ws), nbytes, m, r, d, flags, *cv, _C.stream()), name)
        if train:
            ctx.save_for_backward(xs, saved, *(() if w is None else (w,)))
        ctx.flags, ctx.wshape, ctx.c = flags, None if weights is None else weights.shape, c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        xs, saved, *rest = ctx.saved_tensors
        w = rest[0] if rest else None
        m, r, d = xs.shape
        go = go.to(torch.float32).contiguous()
        gx = torch.empty_like(xs) if ctx.needs_input_grad[0] else None
        gw = torch.empty_like(w) if w is not None and ctx.needs_input_grad[1] else None
        nbytes = _C.lib.hypad_weighted_midpoint_workspace_bytes(m, r, d)
        ws = torch.empty(max(nbytes // 4, 1), device=xs.device, dtype=torch.float32)
        fn, cv, name = _entry("weighted_midpoint_bwd", ctx.c)
        _C.check(fn(_C.ptr(xs), _C.ptr(w), 0 if w is None else w.shape[0], _C.ptr(saved), _C.ptr(go), _C.ptr(gx), _C.ptr(gw), _C.ptr(ws), nbytes, m, r,
                    d, ctx.flags, *cv, _C.stream()), name)
        return gx, None if gw is None else gw.view(ctx.wshape), None, None


_MID_SUPPORTED = ("supported: k = -1, dim = -1, fp32, reducedim among the dimensions of xs before the last, weights None, of one element, or "
                  "broadcastable to xs.shape[:-1], rows of at most 256 elements")


def weighted_midpoint(xs, k, weights=None, reducedim=None, dim=-1, keepdim=False, lincomb=False, posweight=False, coadd=False):
    """The weighted Moebius gyromidpoint (Einstein midpoint in Poincare coordinates) of the points of xs (..., D) over the dimensions
    ``reducedim`` (default: all but the last) (math_.py:1953-2087) at k = -1: the pooling step that turns many ball points into one.
    HIP kernels forward and backward (a wave per kept row, fp64 sums); first-order differentiable in xs and weights.  The reduced
    dimensions are moved to the front and xs is flattened to (reduced, kept, D) -- a copy only where the layout needs one; weights
    that broadcast against xs.shape[:-1] are expanded and materialised, which leaves the sum of their gradient to autograd."""
    _refuse_k("weighted_midpoint", k, _MID_SUPPORTED)
    return _weighted_midpoint(xs, weights, reducedim, dim, keepdim, lincomb, posweight, coadd, _WeightedMidpoint.apply)


def _weighted_midpoint(xs, weights, reducedim, dim, keepdim, lincomb, posweight, coadd, apply):
    """The operand rules of weighted_midpoint, then ``apply(xs3, weights2, flags)``: the k = -1 autograd function, or the one of
    PoincareBall(c) (hyperspace/ball.py)."""
    if xs.dim() < 1 or (dim != -1 and dim != xs.dim() - 1):
        raise NotImplementedError(f"weighted_midpoint: dim = {dim} on xs {tuple(xs.shape)} is not implemented; {_MID_SUPPORTED}")
    nd = xs.dim() - 1
    if reducedim is None:
        red = list(range(nd))
    else:
        red = [reducedim] if isinstance(reducedim, int) else list(reducedim)
        red = sorted({int(a) + xs.dim() if int(a) < 0 else int(a) for a in red})
        if len(red) != len([reducedim] if isinstance(reducedim, int) else list(reducedim)) or any(a < 0 or a >= nd for a in red):
            raise NotImplementedError(f"weighted_midpoint: reducedim = {reducedim} on xs {tuple(xs.shape)} is not implemented; {_MID_SUPPORTED}")
    if xs.dtype != torch.float32 or xs.shape[-1] > 256:
        raise NotImplementedError(f"weighted_midpoint: xs {tuple(xs.shape)} {xs.dtype} is not implemented; {_MID_SUPPORTED}")
    lead = tuple(xs.shape[:-1])
    if weights is not None and weights.numel() != 1:
        try:
            fits = weights.dtype == torch.float32 and tuple(torch.broadcast_shapes(tuple(weights.shape), lead)) == lead
        except RuntimeError:
            fits = False
        if not fits:
            raise NotImplementedError(f"weighted_midpoint: weights {tuple(weights.shape)} {weights.dtype} against xs {tuple(xs.shape)} is not "
                                      f"implemented; {_MID_SUPPORTED}")
    kept = [a for a in range(nd) if a not in red]
    m = 1
    for a in red:
        m *= xs.shape[a]
    if m == 0:
        raise NotImplementedError(f"weighted_midpoint: a midpoint of no points (xs {tuple(xs.shape)}, reducedim {red}) is not implemented")
    r = 1
    for a in kept:
        r *= xs.shape[a]
    order = red + kept
    x3 = xs.permute(*order, nd).reshape(m, r, xs.shape[-1])
    w2 = weights
    if weights is not None and weights.numel() != 1:
        w2 = weights.expand(lead).permute(*order).reshape(m, r)
    flags = (_C.MID_LINCOMB if lincomb else 0) | (_C.MID_POSWEIGHT if posweight else 0) | (_C.MID_COADD if coadd else 0)
    out = apply(x3, w2, flags)
    shape = [1 if a in red else xs.shape[a] for a in range(nd)] if keepdim else [xs.shape[a] for a in kept]
    return out.view(*shape, xs.shape[-1])


class _DistMatmul(torch.autograd.Function):
    """hypad_dist_matmul_* (c given: hypad_ball_dist_matmul_*): x (batch, N, D), y (batch, M, D) -> (batch, N, M); saves the operands alone."""

    @staticmethod
    def forward(ctx, x, y, c=None):
        x = _C.require_cuda(x.contiguous(), "x")
        y = _C.require_cuda(y.contiguous(), "y")
        batch, n, d = x.shape
        m = y.shape[1]
        out = torch.empty(batch, n, m, device=x.device, dtype=torch.float32)
        fn, cv, name = _entry("dist_matmul_fwd", c)
        _C.check(fn(_C.ptr(x), _C.ptr(y), _C.ptr(out), batch, n, m, d, *cv, _C.stream()), name)
        ctx.save_for_backward(x, y)
        ctx.c = c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x, y = ctx.saved_tensors
        batch, n, d = x.shape
        go = go.to(torch.float32).contiguous()
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(y) if ctx.needs_input_grad[1] else None
        fn, cv, name = _entry("dist_matmul_bwd", ctx.c)
        _C.check(fn(_C.ptr(x), _C.ptr(y), _C.ptr(go), _C.ptr(gx), _C.ptr(gy), batch, n, y.shape[1], d, *cv, _C.stream()), name)
        return gx, gy, None


_DISTMM_SUPPORTED = ("supported: k = -1, fp32, x (..., N, D) against y (..., D, M) with the same leading batch dimensions on both, or none on one "
                     "of them, D <= 256, fewer than 2^31 distances")


def dist_matmul(x, y, k):
    """The geodesic distance of every point of x (..., N, D) from every point of y (..., D, M) -> (..., N, M) (math_.py:905-947) at
    k = -1: the score of a hyperbolic attention layer, ``dist_matmul(q, keys.transpose(-1, -2), k)``.  One HIP launch forward on fp32
    MFMA, one fused launch per gradient; first-order differentiable in x and y.  y is handed to the kernels as points (..., M, D): a y
    that is the transposed view of such a tensor is passed as it is, any other is copied once.  Both operands carry the same leading
    batch dimensions, or one of them carries none: that operand is expanded over the batch and materialised on the host, and the sum of
    its gradient over the batch is left to autograd (the expand's backward)."""
    _refuse_k("dist_matmul", k, _DISTMM_SUPPORTED)
    return _dist_matmul(x, y, _DistMatmul.apply)


def _dist_matmul(x, y, apply):
    """The operand rules of dist_matmul, then ``apply(x3, y3)``: the k = -1 autograd function, or the one of PoincareBall(c)
    (hyperspace/ball.py)."""
    bx, by = tuple(x.shape[:-2]), tuple(y.shape[:-2])
    if (x.dim() < 2 or y.dim() < 2 or y.shape[-2] != x.shape[-1] or (bx != by and bx != () and by != ())
            or x.dtype != torch.float32 or y.dtype != torch.float32):
        raise NotImplementedError(f"dist_matmul: x {tuple(x.shape)} {x.dtype} against y {tuple(y.shape)} {y.dtype} is not implemented; "
                                  f"{_DISTMM_SUPPORTED}")
    lead = bx or by
    count = x.shape[-2] * y.shape[-1]
    for n in lead:
        count *= n
    if x.shape[-1] > 256 or x.shape[-1] < 1 or count >= 2 ** 31:
        raise NotImplementedError(f"dist_matmul: x {tuple(x.shape)} against y {tuple(y.shape)} is not implemented; {_DISTMM_SUPPORTED}")
    yt = y.transpose(-1, -2)                                 # (..., M, D): contiguous already in the usual call
    x3, (y3,) = _over_batch(lead, x, (yt,))
    out = apply(x3, y3)
    return out.view(*lead, x.shape[-2], yt.shape[-2])


def _over_batch(lead, x, points):
    """x (..., N, D) and every tensor of ``points`` (..., M, D) as (batch, rows, D) over the leading dimensions ``lead``: an operand
    that carries none of them is expanded (materialised by the autograd function's ``contiguous``; the expand's backward sums its
    gradient over the batch)."""
    nb = 1
    for n in lead:
        nb *= n
    flat = [(t if tuple(t.shape[:-2]) == lead else t.expand(*lead, *t.shape[-2:])) for t in (x, *points)]
    flat = [t.reshape(nb, *t.shape[-2:]) for t in flat]
    return flat[0], flat[1:]


class _Dist2PlaneMatmul(torch.autograd.Function):
    """hypad_dist2plane_matmul_*: x (batch, N, D), p and z (batch, M, D) -> (batch, N, M); saves the operands alone."""

    @staticmethod
    def forward(ctx, x, p, z):
        x = _C.require_cuda(x.contiguous(), "x")
        p = _C.require_cuda(p.contiguous(), "p")
        z = _C.require_cuda(z.contiguous(), "z")
        batch, n, d = x.shape
        m = p.shape[1]
        out = torch.empty(batch, n, m, device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_dist2plane_matmul_fwd(_C.ptr(x), _C.ptr(p), _C.ptr(z), _C.ptr(out), batch, n, m, d, _C.stream()),
                 "dist2plane_matmul_fwd")
        ctx.save_for_backward(x, p, z)
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x, p, z = ctx.saved_tensors
        batch, n, d = x.shape
        go = go.to(torch.float32).contiguous()
        gx, gp, gz = (torch.empty_like(t) if need else None for t, need in zip((x, p, z), ctx.needs_input_grad))
        _C.check(_C.lib.hypad_dist2plane_matmul_bwd(_C.ptr(x), _C.ptr(p), _C.ptr(z), _C.ptr(go), _C.ptr(gx), _C.ptr(gp), _C.ptr(gz), batch, n,
                                                    p.shape[1], d, _C.stream()), "dist2plane_matmul_bwd")
        return gx, gp, gz


_D2PMM_SUPPORTED = ("supported: k = -1, fp32, x (..., N, D) against points p and normals z of one shape (..., D, M), with the same leading batch "
                    "dimensions on x and on the planes, or none on one side, 1 <= D <= 256, fewer than 2^31 elements in the output")


def dist2plane_matmul(x, p, z, *, k):
    """The reference's batched hyperplane read-out (math_.py:2125-2159) at k = -1: x (..., N, D) on the ball against M planes given by
    their points p (..., D, M) on the ball and their normals z (..., D, M) -> (..., N, M), in the operand layout of ``dist_matmul``:
    ``dist2plane_matmul(x, points.transpose(-1, -2), normals.transpose(-1, -2), k=k)``.  With zh = z / max(|z|, 1e-15),

        out = 2 asinh((2 / max(1 - |p|^2, 1e-15)) (<x, zh> - (1 - 2 <x, p> + |x|^2) / max(1 - |x|^2, 1e-15) <p, zh>)) |z|

    This is the reference's formula as it stands.  It is NOT ``2 * dist2plane(x, p, z, signed=True, scaled=True)`` of the transposed
    operands: the two agree only where x = 0 (docs/history/dist2plane_matmul.md).  One HIP launch forward on fp32 MFMA with an fp64
    epilogue, one fused launch for grad_x and one for grad_p and grad_z; first-order differentiable in x, p and z.  The planes are handed
    to the kernels as rows (..., M, D): a p or z that is the transposed view of such a tensor is passed as it is, any other is copied
    once.  x and the planes carry the same leading batch dimensions, or one side carries none: that side is expanded over the batch and
    materialised on the host, and the sum of its gradient over the batch is left to autograd (the expand's backward)."""
    _refuse_k("dist2plane_matmul", k, _D2PMM_SUPPORTED)
    bx, bp = tuple(x.shape[:-2]), tuple(p.shape[:-2])
    if (x.dim() < 2 or p.dim() < 2 or p.shape != z.shape or p.shape[-2] != x.shape[-1] or (bx != bp and bx != () and bp != ())
            or x.dtype != torch.float32 or p.dtype != torch.float32 or z.dtype != torch.float32):
        raise NotImplementedError(f"dist2plane_matmul: x {tuple(x.shape)} {x.dtype} against p {tuple(p.shape)} {p.dtype} and z {tuple(z.shape)} "
                                  f"{z.dtype} is not implemented; {_D2PMM_SUPPORTED}")
    lead = bx or bp
    count = x.shape[-2] * p.shape[-1]
    for n in lead:
        count *= n
    if x.shape[-1] > 256 or x.shape[-1] < 1 or count >= 2 ** 31:
        raise NotImplementedError(f"dist2plane_matmul: x {tuple(x.shape)} against planes {tuple(p.shape)} is not implemented; {_D2PMM_SUPPORTED}")
    x3, (p3, z3) = _over_batch(lead, x, (p.transpose(-1, -2), z.transpose(-1, -2)))
    out = _Dist2PlaneMatmul.apply(x3, p3, z3)
    return out.view(*lead, x.shape[-2], p.shape[-1])


_DIST_SUPPORTED = "supported: k = -1, dim = -1, fp32, x and y of the same shape (nothing is broadcast), rows of 1 to 256 elements"


def _dist_refusals(what, x, k, dim):
    _refuse_k(what, k, _DIST_SUPPORTED)
    if x.dim() < 1 or (dim != -1 and dim != x.dim() - 1):
        raise NotImplementedError(f"{what}: dim = {dim} on x {tuple(x.shape)} is not implemented; {_DIST_SUPPORTED}")
    if x.dtype != torch.float32 or x.shape[-1] > 256 or x.shape[-1] < 1:
        raise NotImplementedError(f"{what}: x {tuple(x.shape)} {x.dtype} is not implemented; {_DIST_SUPPORTED}")


def dist(x, y, *, k, keepdim=False, dim=-1):
    """The geodesic distance 2 artanh(|(-x) (+) y|) of the rows of x from the rows of y (math_.py:861-902) at k = -1: one HIP launch
    forward and one backward, a wave per row; first-order differentiable in x and y.  Rows that are equal element by element are at
    distance 0 with gradient 0."""
    _dist_refusals("dist", x, k, dim)
    if y.shape != x.shape or y.dtype != torch.float32:
        raise NotImplementedError(f"dist: y {tuple(y.shape)} {y.dtype} against x {tuple(x.shape)} is not implemented; {_DIST_SUPPORTED}")
    return _per_row(_RowScalar.apply("dist", None, x, y), keepdim)


def dist0(x, *, k, keepdim=False, dim=-1):
    """The geodesic distance 2 artanh(|x|) of the rows of x from the origin (math_.py:950-975) at k = -1: one HIP launch forward and
    one backward; an all-zero row gets gradient 0."""
    _dist_refusals("dist0", x, k, dim)
    return _per_row(_RowScalar.apply("dist0", None, x), keepdim)


class _HyperbolicAttention(torch.autograd.Function):
    """hypad_hyp_attention_* (c given: hypad_ball_hyp_attention_*): q (batch, N, D), keys (batch, M, D), values (batch, M, E), bias None, (N, M) or (batch, N, M) ->
    (batch, N, E); saves the operands, [nom | den] (batch, N, E + 1) and L (batch, N) -- nothing of size N x M."""

    @staticmethod
    def forward(ctx, q, keys, values, bias, beta, c=None):
        q = _C.require_cuda(q.contiguous(), "q")
        keys = _C.require_cuda(keys.contiguous(), "keys")
        values = _C.require_cuda(values.contiguous(), "values")
        if bias is not None:
            bias = _C.require_cuda(bias.contiguous(), "bias")
        batch, n, d = q.shape
        m, e = values.shape[1], values.shape[2]
        stride = n * m if bias is not None and bias.dim() == 3 else 0
        out = torch.empty(batch, n, e, device=q.device, dtype=torch.float32)
        train = any(ctx.needs_input_grad[:3])
        saved = torch.empty(batch, n, e + 1, device=q.device, dtype=torch.float32) if train else None
        lse = torch.empty(batch, n, device=q.device, dtype=torch.float32) if train else None
        fn, cv, name = _entry("hyp_attention_fwd", c)
        _C.check(fn(_C.ptr(q), _C.ptr(keys), _C.ptr(values), _C.ptr(bias), stride, beta, _C.ptr(out), _C.ptr(saved), _C.ptr(lse), batch, n, m, d, e, *cv,
                    _C.stream()), name)
        if train:
            ctx.save_for_backward(q, keys, values, saved, lse, *(() if bias is None else (bias,)))
        ctx.beta, ctx.stride, ctx.c = beta, stride, c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        q, keys, values, saved, lse, *rest = ctx.saved_tensors
        bias = rest[0] if rest else None
        batch, n, d = q.shape
        m, e = values.shape[1], values.shape[2]
        go = go.to(torch.float32).contiguous()
        gq = torch.empty_like(q) if ctx.needs_input_grad[0] else None
        gk = torch.empty_like(keys) if ctx.needs_input_grad[1] else None
        gv = torch.empty_like(values) if ctx.needs_input_grad[2] else None
        nbytes = _C.lib.hypad_hyp_attention_workspace_bytes(batch, n, m, d, e)
        ws = torch.empty(max(nbytes // 4, 1), device=q.device, dtype=torch.float32)
        fn, cv, name = _entry("hyp_attention_bwd", ctx.c)
        _C.check(fn(_C.ptr(q), _C.ptr(keys), _C.ptr(values), _C.ptr(bias), ctx.stride, ctx.beta, _C.ptr(saved), _C.ptr(lse), _C.ptr(go), _C.ptr(gq),
                    _C.ptr(gk), _C.ptr(gv), _C.ptr(ws), nbytes, batch, n, m, d, e, *cv, _C.stream()), name)
        return gq, gk, gv, None, None, None


_ATTN_SUPPORTED = ("supported: k = -1, fp32, q (..., N, D), keys (..., M, D) and values (..., M, E) with the same leading batch dimensions, or "
                   "none on some of them, 1 <= D, E <= 128, M >= 1, fewer than 2^31 pairs, a finite beta (a float or a one-element tensor) and "
                   "a bias that is None or fp32 (N, M) or (..., N, M), neither of the two requiring grad; for wider rows compose dist_matmul, "
                   "torch.softmax and weighted_midpoint_bmm (D, E <= 256)")


def hyperbolic_attention(q, keys, values, k, beta=1.0, bias=None):
    """Hyperbolic attention at k = -1: for every query of q (..., N, D) the gyromidpoint of the points values (..., M, E) under the
    weights softmax_j(-beta d(q_i, keys_j) + bias_ij), keys (..., M, D) -> (..., N, E).  The contract is the composition of the
    reference's ``dist_matmul(q, keys.transpose(-1, -2), k)`` (math_.py:905-947), ``torch.softmax(-beta * . + bias, -1)`` and
    ``weighted_midpoint_bmm(values, ., k, lincomb=False)`` (math_.py:2090-2122), in one HIP launch forward and three backward that keep
    no (N, M) tensor: the distances and weights are recomputed tile by tile (docs/history/hyperbolic_attention.md).  First-order
    differentiable in q, keys and values; a gradient that is not needed is not computed.

    The three operands carry the same leading batch dimensions, or some carry none: those are expanded over the batch and materialised
    on the host, and the sum of their gradient over the batch is left to autograd.  ``bias`` is fp32 (N, M) -- shared by the batch and
    not expanded -- or (..., N, M); it may hold -inf, the mask, and gets no gradient.  ``beta`` is a finite float or a one-element
    tensor that does not require grad; it is read on the host and handed to the kernels by value, so a captured graph replays the
    value it was captured with, whatever the tensor holds later.

    One difference from the composition: a query whose every score is -inf (a fully masked row) gives the origin, an all-zero row, and
    adds nothing to any gradient; the composition returns NaN there."""
    _refuse_k("hyperbolic_attention", k, _ATTN_SUPPORTED)
    return _hyperbolic_attention(q, keys, values, beta, bias, _HyperbolicAttention.apply)


def _hyperbolic_attention(q, keys, values, beta, bias, apply):
    """The operand rules of hyperbolic_attention, then ``apply(q3, keys3, values3, bias, beta)``: the k = -1 autograd function, or the one
    of PoincareBall(c) (hyperspace/ball.py)."""
    if isinstance(beta, torch.Tensor):
        if beta.numel() != 1 or beta.requires_grad:
            raise NotImplementedError(f"hyperbolic_attention: beta {tuple(beta.shape)} requires_grad={beta.requires_grad} is not implemented; "
                                      f"{_ATTN_SUPPORTED}")
        beta = beta.item()
    beta = float(beta)
    if beta != beta or beta in (float("inf"), float("-inf")):
        raise NotImplementedError(f"hyperbolic_attention: beta = {beta} is not implemented; {_ATTN_SUPPORTED}")
    ops = (q, keys, values)
    desc = ", ".join(f"{n} {tuple(t.shape)} {t.dtype}" for n, t in zip(("q", "keys", "values"), ops))
    if any(t.dim() < 2 or t.dtype != torch.float32 for t in ops):
        raise NotImplementedError(f"hyperbolic_attention: {desc} is not implemented; {_ATTN_SUPPORTED}")
    leads = {tuple(t.shape[:-2]) for t in ops} - {()}
    n, d, m, e = q.shape[-2], q.shape[-1], keys.shape[-2], values.shape[-1]
    if len(leads) > 1 or keys.shape[-1] != d or values.shape[-2] != m or not 1 <= d <= 128 or not 1 <= e <= 128 or m < 1:
        raise NotImplementedError(f"hyperbolic_attention: {desc} is not implemented; {_ATTN_SUPPORTED}")
    lead = leads.pop() if leads else ()
    nb = 1
    for s in lead:
        nb *= s
    if nb * n * m >= 2 ** 31:
        raise NotImplementedError(f"hyperbolic_attention: {desc} ({nb * n * m} pairs) is not implemented; {_ATTN_SUPPORTED}")
    if bias is not None:
        if (bias.dtype != torch.float32 or bias.requires_grad or tuple(bias.shape[-2:]) != (n, m) or bias.dim() < 2
                or tuple(bias.shape[:-2]) not in ((), lead)):
            raise NotImplementedError(f"hyperbolic_attention: bias {tuple(bias.shape)} {bias.dtype} requires_grad={bias.requires_grad} against "
                                      f"{desc} is not implemented; {_ATTN_SUPPORTED}")
        bias = bias if bias.dim() == 2 else bias.reshape(nb, n, m)
    q3, k3, v3 = (t.expand(*lead, *t.shape[-2:]).reshape(nb, *t.shape[-2:]) for t in ops)
    out = apply(q3, k3, v3, bias, beta)
    return out.view(*lead, n, e)


def _row_call(name, direction, c, *args):
    """hypad_<name>_<direction> (c given: hypad_ball_<name>_<direction>, with c before the stream) on the current stream."""
    fn, cv, full = _entry(f"{name}_{direction}", c)
    _C.check(fn(*args, *cv, _C.stream()), f"{name}_{direction}" if c is None else full)


class _RowMap(torch.autograd.Function):
    """hypad_<name>_fwd / _bwd (c given: hypad_ball_<name>_*) for the maps of one to three operands, all of one shape (..., D); saves the
    operands alone."""

    @staticmethod
    def forward(ctx, name, c, *ops):
        ops = [_C.require_cuda(t.contiguous(), f"{name}: operand {i}") for i, t in enumerate(ops)]
        rows, d = _rows_width(ops[0])
        out = torch.empty(ops[0].shape, device=ops[0].device, dtype=torch.float32)
        _row_call(name, "fwd", c, *map(_C.ptr, ops), _C.ptr(out), rows, d)
        ctx.save_for_backward(*ops)
        ctx.name, ctx.c = name, c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        ops = ctx.saved_tensors
        rows, d = _rows_width(ops[0])
        go = go.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) if need else None for t, need in zip(ops, ctx.needs_input_grad[2:])]
        _row_call(ctx.name, "bwd", ctx.c, *map(_C.ptr, ops), _C.ptr(go), *map(_C.ptr, grads), rows, d)
        return (None, None, *grads)


class _TimeRowMap(torch.autograd.Function):
    """hypad_<name>_fwd / _bwd (c given: hypad_ball_<name>_*) for geodesic, geodesic_unit (two row operands (..., D)) and the curved
    mobius_scalar_mul (one): t of one element, or of one element per row."""

    @staticmethod
    def forward(ctx, name, c, t, *ops):
        ops = [_C.require_cuda(a.contiguous(), "x" if i == 0 else f"{name}: the second row operand") for i, a in enumerate(ops)]
        t1 = _C.require_cuda(t.contiguous().reshape(-1), "t")
        rows, d = _rows_width(ops[0])
        out = torch.empty_like(ops[0])
        _row_call(name, "fwd", c, _C.ptr(t1), *map(_C.ptr, ops), _C.ptr(out), rows, d, t1.shape[0])
        ctx.save_for_backward(t1, *ops)
        ctx.name, ctx.c, ctx.ts = name, c, t.shape
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        t1, *ops = ctx.saved_tensors
        rows, d = _rows_width(ops[0])
        go = go.to(torch.float32).contiguous()
        gt = torch.empty(rows, device=ops[0].device, dtype=torch.float32) if ctx.needs_input_grad[2] else None
        grads = [torch.empty_like(a) if need else None for a, need in zip(ops, ctx.needs_input_grad[3:])]
        _row_call(ctx.name, "bwd", ctx.c, _C.ptr(t1), *map(_C.ptr, ops), _C.ptr(go), _C.ptr(gt), *map(_C.ptr, grads), rows, d, t1.shape[0])
        if gt is not None and t1.shape[0] == 1 and rows != 1:   # one t for every row: the rows' contributions, added in a fixed order
            gt = _column_sum(gt.view(rows, 1))
        return (None, None, None if gt is None else gt.view(ctx.ts), *grads)


class _RowScalar(torch.autograd.Function):
    """hypad_<name>_fwd / _bwd (c given: hypad_ball_<name>_*) for lambda_x, norm, inner, dist and dist0: one to three operands of one
    shape (..., D) -> (...), one value per row."""

    @staticmethod
    def forward(ctx, name, c, *ops):
        ops = [_C.require_cuda(t.contiguous(), f"{name}: operand {i}") for i, t in enumerate(ops)]
        rows, d = _rows_width(ops[0])
        out = torch.empty(ops[0].shape[:-1], device=ops[0].device, dtype=torch.float32)
        _row_call(name, "fwd", c, *map(_C.ptr, ops), _C.ptr(out), rows, d)
        ctx.save_for_backward(*ops)
        ctx.name, ctx.c = name, c
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        ops = ctx.saved_tensors
        rows, d = _rows_width(ops[0])
        go = go.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) if need else None for t, need in zip(ops, ctx.needs_input_grad[2:])]
        _row_call(ctx.name, "bwd", ctx.c, *map(_C.ptr, ops), _C.ptr(go), *map(_C.ptr, grads), rows, d)
        return (None, None, *grads)


class _Projection(torch.autograd.Function):
    """hypad_sproj_* (grow = -1) and hypad_inv_sproj_* (grow = +1), or with c their hypad_ball_* forms: a (..., W) -> (..., W + grow); the
    entry points take the ball's width."""

    @staticmethod
    def forward(ctx, name, c, a, grow):
        a = _C.require_cuda(a.contiguous(), name)
        rows, w = _rows_width(a)
        ball = w if grow > 0 else w - 1
        out = torch.empty(*a.shape[:-1], w + grow, device=a.device, dtype=torch.float32)
        _row_call(name, "fwd", c, _C.ptr(a), _C.ptr(out), rows, ball)
        ctx.save_for_backward(a)
        ctx.name, ctx.c, ctx.ball = name, c, ball
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        (a,) = ctx.saved_tensors
        go = go.to(torch.float32).contiguous()
        ga = torch.empty_like(a)
        _row_call(ctx.name, "bwd", ctx.c, _C.ptr(a), _C.ptr(go), _C.ptr(ga), _rows_width(a)[0], ctx.ball)
        return None, None, ga, None


_TANGENT_SUPPORTED = ("supported: k = -1, dim = -1, fp32, operands of the same last dimension whose leading dimensions broadcast against "
                      "each other, rows of 1 to 256 elements, fewer than 2^31 elements")


def _tangent_operands(what, k, dim, **ops):
    """The operands of a tangent map, broadcast against each other by torch's rules (expanded views: a broadcast operand's gradient is
    summed by autograd, the expand's backward); every refusal comes before any device call."""
    _refuse_k(what, k, _TANGENT_SUPPORTED)
    desc = ", ".join(f"{n} {tuple(t.shape)} {t.dtype}" for n, t in ops.items())
    ts = list(ops.values())
    if any(t.dim() < 1 or t.dtype != torch.float32 or t.shape[-1] != ts[0].shape[-1] for t in ts) or not 1 <= ts[0].shape[-1] <= 256:
        raise NotImplementedError(f"{what}: {desc} is not implemented; {_TANGENT_SUPPORTED}")
    try:
        shape = torch.broadcast_shapes(*(tuple(t.shape) for t in ts))
    except RuntimeError:
        raise NotImplementedError(f"{what}: {desc} do not broadcast against each other; {_TANGENT_SUPPORTED}") from None
    if dim != -1 and dim != len(shape) - 1:
        raise NotImplementedError(f"{what}: dim = {dim} on {desc} is not implemented; {_TANGENT_SUPPORTED}")
    count = 1
    for n in shape:
        count *= n
    if count >= 2 ** 31:
        raise NotImplementedError(f"{what}: {desc} ({count} elements) is not implemented; {_TANGENT_SUPPORTED}")
    return torch.broadcast_tensors(*ts)


def _time_operand(what, t, x):
    """(t, x) with t of geodesic and geodesic_unit as a tensor: a number, one element, or one value per row of the broadcast x."""
    if not isinstance(t, torch.Tensor):
        t = torch.tensor(float(t), dtype=torch.float32, device=x.device)
    if t.dtype != torch.float32 or (t.numel() != 1 and tuple(t.shape) != tuple(x.shape[:-1]) + (1,)):
        raise NotImplementedError(f"{what}: t {tuple(t.shape)} {t.dtype} against row operands broadcast to {tuple(x.shape)} is not implemented; "
                                  f"{_TANGENT_SUPPORTED}, t a number, of one element or of shape x.shape[:-1] + (1,)")
    return t, x


def expmap(x, u, *, k, dim=-1):
    """The exponential map at x: the point reached from x along the tangent vector u, x (+) (tanh(lambda_x |u| / 2) u / |u|)
    (math_.py:1052-1102) at k = -1.  One HIP launch forward and one backward, a wave per row in fp64 registers; first-order
    differentiable in x and u, which are broadcast against each other."""
    return _RowMap.apply("expmap", None, *_tangent_operands("expmap", k, dim, x=x, u=u))


def logmap(x, y, *, k, dim=-1):
    """The logarithmic map at x: the tangent vector at x that points to y, 2 artanh(|w|) w / (lambda_x |w|) with w = (-x) (+) y
    (math_.py:1188-1230) at k = -1.  One HIP launch forward and one backward; first-order differentiable in x and y, which are broadcast
    against each other: ``logmap(centroid (B, 1, D), xs (B, N, D))`` maps a batch into the tangent space at its centroid.

    The one deliberate difference from the reference: artanh is 0.5 (log1p(n) - log1p(-n)), so at coincident or near-coincident points
    the result and its gradient follow the analytic limit artanh(n) / n -> 1, where the reference's fp32 run -- a difference of two
    logarithms -- returns a gradient of exactly 0.  There is no singularity at x == y and no special case for it."""
    return _RowMap.apply("logmap", None, *_tangent_operands("logmap", k, dim, x=x, y=y))


def geodesic(t, x, y, *, k, dim=-1):
    """The point at time t of the geodesic from x (t = 0) to y (t = 1), x (+) (t (x) ((-x) (+) y)) (math_.py:978-1049) at k = -1.  One
    HIP launch forward and one backward; first-order differentiable in t, x and y.  x and y are broadcast against each other; t is a
    number, a tensor of one element, or holds one value per row, shape x.shape[:-1] + (1,) after that broadcast.

    As in logmap, artanh is the log1p form: at coincident or near-coincident x and y the result and its gradients follow the analytic
    limit, where the reference's fp32 run returns a gradient of exactly 0."""
    x, y = _tangent_operands("geodesic", k, dim, x=x, y=y)
    return _TimeRowMap.apply("geodesic", None, *_time_operand("geodesic", t, x), y)


def gyration(a, b, u, *, k, dim=-1):
    """The gyration gyr[a, b] u = -(a (+) b) (+) (a (+) (b (+) u)) in its closed form (math_.py:592-675) at k = -1.  One HIP launch
    forward and one backward; first-order differentiable in a, b and u, which are broadcast against each other."""
    return _RowMap.apply("gyration", None, *_tangent_operands("gyration", k, dim, a=a, b=b, u=u))


def parallel_transport(x, y, v, *, k, dim=-1):
    """The parallel transport of the tangent vector v from x to y along their geodesic, gyr[y, -x] v lambda_x / lambda_y
    (math_.py:1669-1746) at k = -1.  One HIP launch forward and one backward; first-order differentiable in x, y and v, which are
    broadcast against each other."""
    return _RowMap.apply("parallel_transport", None, *_tangent_operands("parallel_transport", k, dim, x=x, y=y, v=v))


def parallel_transport0(y, v, *, k, dim=-1):
    """The parallel transport of v from the origin to y, v (1 - |y|^2) (math_.py:1749-1779) at k = -1.  One HIP launch forward and one
    backward; first-order differentiable in y and v, which are broadcast against each other."""
    return _RowMap.apply("parallel_transport0", None, *_tangent_operands("parallel_transport0", k, dim, y=y, v=v))


def parallel_transport0back(x, v, *, k, dim=-1):
    """The parallel transport of v from x to the origin, v / (1 - |x|^2) (math_.py:1782-1813) at k = -1.  One HIP launch forward and one
    backward; first-order differentiable in x and v, which are broadcast against each other."""
    return _RowMap.apply("parallel_transport0back", None, *_tangent_operands("parallel_transport0back", k, dim, x=x, v=v))


def mobius_sub(x, y, *, k, dim=-1):
    """The Moebius subtraction x (+) (-y) (math_.py:558-589) at k = -1.  One HIP launch forward and one backward; first-order
    differentiable in x and y, which are broadcast against each other."""
    return _RowMap.apply("mobius_sub", None, *_tangent_operands("mobius_sub", k, dim, x=x, y=y))


def mobius_coadd(x, y, *, k, dim=-1):
    """The Moebius coaddition ((1 - |y|^2) x + (1 - |x|^2) y) / (1 - |x|^2 |y|^2), the commutative sum of the gyrogroup
    (math_.py:678-744) at k = -1.  One HIP launch forward and one backward; first-order differentiable in x and y, which are broadcast
    against each other."""
    return _RowMap.apply("mobius_coadd", None, *_tangent_operands("mobius_coadd", k, dim, x=x, y=y))


def mobius_cosub(x, y, *, k, dim=-1):
    """The Moebius cosubtraction mobius_coadd(x, -y) (math_.py:747-779) at k = -1: ``mobius_cosub(mobius_add(x, y), y) = x``.  One HIP
    launch forward and one backward; first-order differentiable in x and y, which are broadcast against each other."""
    return _RowMap.apply("mobius_cosub", None, *_tangent_operands("mobius_cosub", k, dim, x=x, y=y))


def geodesic_unit(t, x, u, *, k, dim=-1):
    """The point at geodesic distance t from x in the direction of the tangent vector u, x (+) (tanh(t / 2) u / |u|)
    (math_.py:1139-1185) at k = -1.  One HIP launch forward and one backward; first-order differentiable in t, x and u.  x and u are
    broadcast against each other; t is a number, a tensor of one element, or holds one value per row, shape x.shape[:-1] + (1,) after
    that broadcast."""
    x, u = _tangent_operands("geodesic_unit", k, dim, x=x, u=u)
    return _TimeRowMap.apply("geodesic_unit", None, *_time_operand("geodesic_unit", t, x), u)


def _per_row(out, keepdim):
    return out.unsqueeze(-1) if keepdim else out


def lambda_x(x, *, k, keepdim=False, dim=-1):
    """The conformal factor lambda_x = 2 / (1 - |x|^2) of the rows of x (math_.py:355-383) at k = -1 -> x.shape[:-1], or
    x.shape[:-1] + (1,) with keepdim.  One HIP launch forward and one backward."""
    return _per_row(_RowScalar.apply("lambda_x", None, *_tangent_operands("lambda_x", k, dim, x=x)), keepdim)


def inner(x, u, v, *, k, keepdim=False, dim=-1):
    """The Riemannian inner product lambda_x^2 <u, v> of the tangent vectors u and v at x (math_.py:386-430) at k = -1, one value per
    row.  One HIP launch forward and one backward; first-order differentiable in x, u and v, which are broadcast against each other.

    One deliberate difference from the reference: with keepdim=False the result has the shape x.shape[:-1] (after the broadcast), as
    lambda_x, norm and dist have.  The reference multiplies lambda_x^2 of shape (..., 1) with a sum of shape (...), which broadcasts the
    rows against each other: (33, 5) operands give (33, 33) there.  With keepdim=True the two agree."""
    return _per_row(_RowScalar.apply("inner", None, *_tangent_operands("inner", k, dim, x=x, u=u, v=v)), keepdim)


def norm(x, u, *, k, keepdim=False, dim=-1):
    """The Riemannian norm lambda_x |u| of the tangent vector u at x (math_.py:433-472) at k = -1, one value per row.  One HIP launch
    forward and one backward; first-order differentiable in x and u, which are broadcast against each other; a zero tangent gets
    gradient 0."""
    return _per_row(_RowScalar.apply("norm", None, *_tangent_operands("norm", k, dim, x=x, u=u)), keepdim)


def egrad2rgrad(x, grad, *, k, dim=-1):
    """The Riemannian gradient at x of a function whose Euclidean gradient there is ``grad``: grad / lambda_x^2 (math_.py:1816-1845) at
    k = -1.  ``p <- expmap(p, -lr * egrad2rgrad(p, p.grad))`` is one step of Riemannian gradient descent.  One HIP launch forward and one
    backward; first-order differentiable in x and grad, which are broadcast against each other."""
    return _RowMap.apply("egrad2rgrad", None, *_tangent_operands("egrad2rgrad", k, dim, x=x, grad=grad))


_PROJ_SUPPORTED = ("supported: k = -1, dim = -1, fp32, a ball side of 1 to 255 elements a row (the hyperboloid side, one more, of 2 to 256), fewer "
                   "than 2^31 elements")


def _projection_refusals(what, a, k, dim, grow):
    _refuse_k(what, k, _PROJ_SUPPORTED)
    if a.dim() < 1 or (dim != -1 and dim != a.dim() - 1):
        raise NotImplementedError(f"{what}: dim = {dim} on {tuple(a.shape)} is not implemented; {_PROJ_SUPPORTED}")
    rows, wide = _rows_width(a)[0], a.shape[-1] + max(grow, 0)            # the hyperboloid side
    if a.dtype != torch.float32 or not 2 <= wide <= 256 or rows * wide >= 2 ** 31:
        raise NotImplementedError(f"{what}: {tuple(a.shape)} {a.dtype} is not implemented; {_PROJ_SUPPORTED}")


def sproj(x, *, k, dim=-1):
    """The stereographic projection of hyperboloid points x (..., D + 1), the time-like coordinate last, onto the ball:
    x[..., :D] / (1 + x[..., D]) (math_.py:1848-1874) at k = -1, where the reference's inv_r = sqrt(|k| + 1e-15) is 1.  No clamp, as in the
    reference.  One HIP launch forward and one backward."""
    _projection_refusals("sproj", x, k, dim, -1)
    return _Projection.apply("sproj", None, x, -1)


def inv_sproj(x, *, k, dim=-1):
    """The inverse stereographic projection of ball points x (..., D) onto the hyperboloid: cat(lambda_x x, lambda_x - 1), shape
    (..., D + 1) (math_.py:1877-1905) at k = -1.  One HIP launch forward and one backward."""
    _projection_refusals("inv_sproj", x, k, dim, 1)
    return _Projection.apply("inv_sproj", None, x, 1)


def antipode(x, *, k, dim=-1):
    """The antipode of x (math_.py:1908-1950): -x for every k <= 0, as the reference returns.  No kernel."""
    _refuse_k("antipode", k, "supported: k = -1")
    return -x


def mobius_fn_apply_chain(x, *fns, k=None, dim=-1):
    """expmap0(fn_n(... fn_1(logmap0(x)))) (math_.py:1374-1428): the two maps are the HIP kernels above, the functions are the caller's
    own.  Without a function it returns x."""
    _check_k(k)
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError("mobius_fn_apply_chain: only the last dimension (dim = -1) is implemented")
    if not fns:
        return x
    ex = logmap0(x)
    for fn in fns:
        ex = fn(ex)
    return expmap0(ex)


def mobiusify(fn):
    """``fn`` wrapped to work on ball points (math_.py:1472-1498): the new function takes ``k`` and ``dim`` and is
    mobius_fn_apply(fn, x, *args, k=k, dim=dim, **kwargs)."""
    import functools

    @functools.wraps(fn)
    def mobius_fn(x, *args, k=None, dim=-1, **kwargs):
        return mobius_fn_apply(fn, x, *args, k=k, dim=dim, **kwargs)
    return mobius_fn


def mobius_fn_apply(fn, x, *args, k=None, dim=-1, **kwargs):
    """expmap0(fn(logmap0(x)))  (math_.py:1431-1469): the two maps are the HIP kernels above (first-order gradients, as theirs);
    ``fn`` is the caller's own function of the tangent vector.  Inside mobius_linear, tanh and relu run fused in the layer's
    kernels instead (hyrnn_nets.mobius_linear).  A floating x of any dtype is cast to fp32 by logmap0: ``fn`` sees fp32, and the result
    is fp32."""
    _check_k(k)
    _check_last_dim("mobius_fn_apply", x, dim)
    return expmap0(fn(logmap0(x), *args, **kwargs))


def mobius_matvec(m, x, *, k=None, dim=-1):
    """math_.py:1308-1323: see hyrnn_nets.mobius_matvec (one HIP launch, differentiable in m and x; a floating x of any dtype is cast to
    fp32, m is fp32, the result is fp32)."""
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
    differentiable in x, p and a.  A floating x of any dtype is cast to fp32; p and a are fp32, and so is the result."""
    _refuse_k("dist2plane", k, _D2P_SUPPORTED)
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
        _launch(u2.shape[0], "hypad_poincare_rowdist_fwd", _C.ptr(u2), _C.ptr(v2), _C.ptr(out), u2.shape[0], u2.shape[1], _C.stream())
        ctx.save_for_backward(u2, v2)
        ctx.us, ctx.vs = u.shape, v.shape
        return out.view(u.shape[:-1])

    @staticmethod
    @_C.first_order_only
    def backward(ctx, gd):
        u2, v2 = ctx.saved_tensors
        gd = gd.to(torch.float32).contiguous().reshape(-1)
        gu, gv = torch.empty_like(u2), torch.empty_like(v2)
        _launch(u2.shape[0], "hypad_poincare_rowdist_bwd", _C.ptr(u2), _C.ptr(v2), _C.ptr(gd), _C.ptr(gu), _C.ptr(gv), u2.shape[0], u2.shape[1],
                _C.stream())
        return gu.view(ctx.us), gv.view(ctx.vs)


def poincare_rowdist(u, v):
    """acosh(1 + 2|u-v|^2 / ((1-|u|^2)(1-|v|^2)) + 1e-7) per row (train.py:226-230).  u and v have one shape (..., D); floating operands
    of any dtype are cast to fp32 (the fp64 window path of utils/anomaly_detection_utils.py relies on it) and the result is fp32."""
    return _RowDist.apply(u, v)


class _HyperLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, v, batch):
        _same_shape("hyperbolic_loss", u, v)
        u, u2 = _rows(u)
        v, v2 = _rows(v)
        out = torch.empty(1, device=u2.device, dtype=torch.float32) if u2.shape[0] else torch.zeros(1, device=u2.device, dtype=torch.float32)
        _launch(u2.shape[0], "hypad_hyper_loss_fwd", _C.ptr(u2), _C.ptr(v2), _C.ptr(out), u2.shape[0], u2.shape[1], int(batch), _C.stream())
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
    """torch.div(torch.sum(dist), batch_size)  (train.py:232); 0 over no rows.  Floating operands of any dtype are cast to fp32 and the
    result is fp32."""
    return _HyperLoss.apply(u, v, batch_size)
