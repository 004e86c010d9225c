"""MobiusLinear / mobius_linear / mobius_matvec, the Moebius GRU and MobiusDist2Hyperplane on the GPU (reference:
hyperspace/hyrnn_nets.py:13-58, :61-151, :154-200, :210-245).

Every configuration of the layer runs as one fused HIP forward launch and a HIP backward: Euclidean or ball-valued
input (the latter through the Moebius matrix-vector product), ball-valued, Euclidean or no bias, and no
non-linearity, tanh or relu.  The configuration the hot path uses (Euclidean input, ball-valued bias, no
non-linearity: models/tadgan.py:43-52) keeps its own entry points.  k = -1 and fp32 only; anything else raises.

The GRU (one_rnn_transform, mobius_gru_cell, mobius_gru_loop) carries a hidden state on the ball through time: one GEMM for the input
projection of all steps, one launch for the whole recurrence, one persistent launch for back-propagation through time
(csrc/mobius_gru.hip).  The reference file has no module around it, and neither has this one.
"""
import math

import torch
from torch import nn

from .. import _C


class PoincareBall:
    """The Poincare ball of curvature k = -c (the reference's geoopt.PoincareBall(c)): the tag of ball-valued parameters, and the
    object through which the 25 row-wise functions of math_.py and ``antipode`` are reached with k = -c bound -- ``ball.expmap(x, u)``,
    ``ball.dist(x, y)``, ``ball.transp(x, y, v)`` -- under the names of math_.py and geoopt's aliases ``projx``, ``transp``, ``transp0``
    and ``transp0back``; and ``dist_matmul``, ``weighted_midpoint``, ``weighted_midpoint_bmm`` and ``hyperbolic_attention``, the k = -1
    kernels with c in their fp64 stages (docs/history/curvature_matmul.md).

    Each method takes the operands of the ``gmath`` function of its name without ``k`` and applies that function's operand rules and
    refusals before any device call.  The refusals are ``gmath``'s own and carry its text, "supported: k = -1, ...": read through a ball
    of another c, everything after "k = -1" in that list is the rule here too, and the curvature is the ball's.  At c == 1 a method
    calls that function, so its bits are ``gmath``'s; at any other finite c > 0 it runs the ``hypad_ball_*`` kernels, one HIP launch forward and one backward, a wave per row in fp64 registers (hyperspace/ball.py,
    docs/history/curvature.md).  c <= 0, a c that is not finite and a c that requires grad raise NotImplementedError.  c is read on
    the host from the tensor stored here: nothing waits for the device, the launches go to the current stream and can be captured
    under ``torch.cuda.graph`` (a replay uses the c it was captured with).

    The methods are the functions of math_.py and nothing more: unlike geoopt's manifold class none of them projects its result back
    into the ball implicitly (geoopt's ``expmap(..., project=True)``, ``mobius_add(..., project=True)``); call ``project`` where it is
    wanted (weighted_midpoint_bmm and hyperbolic_attention project because the reference's functions do).  dist2plane,
    dist2plane_matmul, the Moebius layers and GRU, and the optimisers stay at c = 1."""

    def __init__(self, c=1.0):
        self.c = torch.tensor(float(c))
        self.k = -self.c

    def _c(self, what):
        from . import ball
        return ball.curvature(self, what)

    # ---- one operand
    def project(self, x, *, dim=-1, eps=-1.0):
        """Rows beyond the norm (1 - 4e-3) / sqrt(c) scaled back onto it (math_.py:340-352)."""
        from . import ball, gmath
        c = self._c("project")
        if eps >= 0:
            raise NotImplementedError("custom eps: the fused kernel uses the fp32 default 4e-3 (math_.py:343-347)")
        ball.cast_rows("project", dim, x=x)
        return gmath.project(x, k=-1.0, dim=dim) if c == 1.0 else ball.unary("project", c, x, dim)

    def expmap0(self, u, *, dim=-1):
        """tanh(sqrt(c) |u|) u / (sqrt(c) |u|) (math_.py:1105-1136)."""
        from . import ball, gmath
        c = self._c("expmap0")
        ball.cast_rows("expmap0", dim, u=u)
        return gmath.expmap0(u, k=-1.0, dim=dim) if c == 1.0 else ball.unary("expmap0", c, u, dim)

    def logmap0(self, y, *, dim=-1):
        """artanh(sqrt(c) |y|) y / (sqrt(c) |y|) (math_.py:1233-1270)."""
        from . import ball, gmath
        c = self._c("logmap0")
        ball.cast_rows("logmap0", dim, y=y)
        return gmath.logmap0(y, k=-1.0, dim=dim) if c == 1.0 else ball.unary("logmap0", c, y, dim)

    def dist0(self, x, *, keepdim=False, dim=-1):
        """The geodesic distance from the origin, 2 artanh(sqrt(c) |x|) / sqrt(c) (math_.py:950-975)."""
        from . import ball, gmath
        c = self._c("dist0")
        return gmath.dist0(x, k=-1.0, keepdim=keepdim, dim=dim) if c == 1.0 else ball.dist0(c, x, keepdim, dim)

    def lambda_x(self, x, *, keepdim=False, dim=-1):
        """The conformal factor 2 / (1 - c |x|^2) (math_.py:355-383)."""
        from . import ball, gmath
        c = self._c("lambda_x")
        return gmath.lambda_x(x, k=-1.0, keepdim=keepdim, dim=dim) if c == 1.0 else ball.per_row("lambda_x", c, keepdim, dim, x=x)

    def sproj(self, x, *, dim=-1):
        """Hyperboloid points (..., D + 1) onto the ball: x[..., :D] / (1 + sqrt(c) x[..., D]) (math_.py:1848-1874)."""
        from . import ball, gmath
        c = self._c("sproj")
        return gmath.sproj(x, k=-1.0, dim=dim) if c == 1.0 else ball.projection("sproj", c, x, dim, -1)

    def inv_sproj(self, x, *, dim=-1):
        """Ball points (..., D) onto the hyperboloid: cat(lambda_x x, (lambda_x - 1) / sqrt(c)) (math_.py:1877-1905)."""
        from . import ball, gmath
        c = self._c("inv_sproj")
        return gmath.inv_sproj(x, k=-1.0, dim=dim) if c == 1.0 else ball.projection("inv_sproj", c, x, dim, 1)

    def antipode(self, x, *, dim=-1):
        """-x, the antipode at every k < 0 (math_.py:1908-1950).  No kernel."""
        self._c("antipode")
        return -x

    # ---- two ball points, or a point and a tangent vector
    def mobius_add(self, x, y, *, dim=-1):
        """x (+) y at curvature -c (math_.py:536-555); x and y broadcast against each other."""
        from . import ball, gmath
        c = self._c("mobius_add")
        ball.cast_rows("mobius_add", dim, x=x, y=y)
        return gmath.mobius_add(x, y, k=-1.0, dim=dim) if c == 1.0 else ball.mobius_add(c, x, y, dim)

    def mobius_sub(self, x, y, *, dim=-1):
        """x (+) (-y) (math_.py:558-589)."""
        from . import ball, gmath
        c = self._c("mobius_sub")
        return gmath.mobius_sub(x, y, k=-1.0, dim=dim) if c == 1.0 else ball.rows("mobius_sub", c, dim, x=x, y=y)

    def mobius_coadd(self, x, y, *, dim=-1):
        """The Moebius coaddition (math_.py:678-744)."""
        from . import ball, gmath
        c = self._c("mobius_coadd")
        return gmath.mobius_coadd(x, y, k=-1.0, dim=dim) if c == 1.0 else ball.rows("mobius_coadd", c, dim, x=x, y=y)

    def mobius_cosub(self, x, y, *, dim=-1):
        """mobius_coadd(x, -y) (math_.py:747-779)."""
        from . import ball, gmath
        c = self._c("mobius_cosub")
        return gmath.mobius_cosub(x, y, k=-1.0, dim=dim) if c == 1.0 else ball.rows("mobius_cosub", c, dim, x=x, y=y)

    def dist(self, x, y, *, keepdim=False, dim=-1):
        """The geodesic distance 2 artanh(sqrt(c) |(-x) (+) y|) / sqrt(c) (math_.py:861-902); rows that are equal element by element are
        at distance 0 with gradient 0."""
        from . import ball, gmath
        c = self._c("dist")
        return gmath.dist(x, y, k=-1.0, keepdim=keepdim, dim=dim) if c == 1.0 else ball.dist(c, x, y, keepdim, dim)

    def expmap(self, x, u, *, dim=-1):
        """The exponential map at x (math_.py:1052-1102)."""
        from . import ball, gmath
        c = self._c("expmap")
        return gmath.expmap(x, u, k=-1.0, dim=dim) if c == 1.0 else ball.rows("expmap", c, dim, x=x, u=u)

    def logmap(self, x, y, *, dim=-1):
        """The logarithmic map at x (math_.py:1188-1230), with the library's log1p artanh: at coincident points it follows the analytic
        limit, as ``gmath.logmap``."""
        from . import ball, gmath
        c = self._c("logmap")
        return gmath.logmap(x, y, k=-1.0, dim=dim) if c == 1.0 else ball.rows("logmap", c, dim, x=x, y=y)

    def parallel_transport0(self, y, v, *, dim=-1):
        """The parallel transport of v from the origin to y, v (1 - c |y|^2) (math_.py:1749-1779)."""
        from . import ball, gmath
        c = self._c("parallel_transport0")
        return gmath.parallel_transport0(y, v, k=-1.0, dim=dim) if c == 1.0 else ball.rows("parallel_transport0", c, dim, y=y, v=v)

    def parallel_transport0back(self, x, v, *, dim=-1):
        """The parallel transport of v from x to the origin, v / (1 - c |x|^2) (math_.py:1782-1813)."""
        from . import ball, gmath
        c = self._c("parallel_transport0back")
        return gmath.parallel_transport0back(x, v, k=-1.0, dim=dim) if c == 1.0 else ball.rows("parallel_transport0back", c, dim, x=x, v=v)

    def norm(self, x, u, *, keepdim=False, dim=-1):
        """The Riemannian norm lambda_x |u| (math_.py:433-472)."""
        from . import ball, gmath
        c = self._c("norm")
        return gmath.norm(x, u, k=-1.0, keepdim=keepdim, dim=dim) if c == 1.0 else ball.per_row("norm", c, keepdim, dim, x=x, u=u)

    def egrad2rgrad(self, x, grad, *, dim=-1):
        """The Riemannian gradient grad / lambda_x^2 (math_.py:1816-1845)."""
        from . import ball, gmath
        c = self._c("egrad2rgrad")
        return gmath.egrad2rgrad(x, grad, k=-1.0, dim=dim) if c == 1.0 else ball.rows("egrad2rgrad", c, dim, x=x, grad=grad)

    # ---- a scalar or a weight row with a point
    def mobius_scalar_mul(self, r, x, *, dim=-1):
        """r (x) x = tanh(r artanh(sqrt(c) |x|)) x / (sqrt(c) |x|) (math_.py:788-858); r a number, one element, or one value per row."""
        from . import ball, gmath
        c = self._c("mobius_scalar_mul")
        return gmath.mobius_scalar_mul(r, x, k=-1.0, dim=dim) if c == 1.0 else ball.mobius_scalar_mul(c, r, x, dim)

    def mobius_pointwise_mul(self, w, x, *, dim=-1):
        """diag(w) (x) x (math_.py:1328-1371); w of the shape of x or one row of it."""
        from . import ball, gmath
        c = self._c("mobius_pointwise_mul")
        return gmath.mobius_pointwise_mul(w, x, k=-1.0, dim=dim) if c == 1.0 else ball.mobius_pointwise_mul(c, w, x, dim)

    # ---- three operands
    def geodesic(self, t, x, y, *, dim=-1):
        """The point at time t of the geodesic from x to y (math_.py:978-1049); t a number, one element, or one value per row."""
        from . import ball, gmath
        c = self._c("geodesic")
        return gmath.geodesic(t, x, y, k=-1.0, dim=dim) if c == 1.0 else ball.timed("geodesic", c, t, dim, x=x, y=y)

    def geodesic_unit(self, t, x, u, *, dim=-1):
        """The point at geodesic distance t from x in the direction u (math_.py:1139-1185)."""
        from . import ball, gmath
        c = self._c("geodesic_unit")
        return gmath.geodesic_unit(t, x, u, k=-1.0, dim=dim) if c == 1.0 else ball.timed("geodesic_unit", c, t, dim, x=x, u=u)

    def gyration(self, a, b, u, *, dim=-1):
        """gyr[a, b] u (math_.py:592-675)."""
        from . import ball, gmath
        c = self._c("gyration")
        return gmath.gyration(a, b, u, k=-1.0, dim=dim) if c == 1.0 else ball.rows("gyration", c, dim, a=a, b=b, u=u)

    def parallel_transport(self, x, y, v, *, dim=-1):
        """The parallel transport of v from x to y along their geodesic (math_.py:1669-1746)."""
        from . import ball, gmath
        c = self._c("parallel_transport")
        return gmath.parallel_transport(x, y, v, k=-1.0, dim=dim) if c == 1.0 else ball.rows("parallel_transport", c, dim, x=x, y=y, v=v)

    def inner(self, x, u, v, *, keepdim=False, dim=-1):
        """The Riemannian inner product lambda_x^2 <u, v>, one value per row as ``gmath.inner`` (math_.py:386-430)."""
        from . import ball, gmath
        c = self._c("inner")
        return gmath.inner(x, u, v, k=-1.0, keepdim=keepdim, dim=dim) if c == 1.0 else ball.per_row("inner", c, keepdim, dim, x=x, u=u, v=v)

    # ---- the matmul forms and what is built on them (docs/history/curvature_matmul.md)
    def dist_matmul(self, x, y):
        """The geodesic distance at curvature -c of every point of x (..., N, D) from every point of y (..., D, M) -> (..., N, M)
        (math_.py:905-947); a coincident pair is at (2 / sqrt(c)) artanh(sqrt(c) sqrt(1e-15)) = 6.3e-8, the reference's floor."""
        from . import ball, gmath
        c = self._c("dist_matmul")
        return gmath.dist_matmul(x, y, -1.0) if c == 1.0 else ball.dist_matmul(c, x, y)

    def weighted_midpoint(self, xs, weights=None, reducedim=None, dim=-1, keepdim=False, lincomb=False, posweight=False, coadd=False):
        """The weighted gyromidpoint at curvature -c of the points of xs (..., D) over ``reducedim`` (math_.py:1953-2087): the pooling
        form, which does not project."""
        from . import ball, gmath
        c = self._c("weighted_midpoint")
        if c == 1.0:
            return gmath.weighted_midpoint(xs, -1.0, weights, reducedim, dim, keepdim, lincomb, posweight, coadd)
        return ball.weighted_midpoint(c, xs, weights, reducedim, dim, keepdim, lincomb, posweight, coadd)

    def weighted_midpoint_bmm(self, xs, weights, lincomb=False):
        """The weighted gyromidpoint at curvature -c of xs (..., M, D) under every row of weights (..., N, M) -> (..., N, D)
        (math_.py:2090-2122), projected onto the radius (1 - 4e-3) / sqrt(c)."""
        from . import ball, gmath
        c = self._c("weighted_midpoint_bmm")
        return gmath.weighted_midpoint_bmm(xs, weights, -1.0, lincomb) if c == 1.0 else ball.weighted_midpoint_bmm(c, xs, weights, lincomb)

    def hyperbolic_attention(self, q, keys, values, beta=1.0, bias=None):
        """Per query of q (..., N, D) the gyromidpoint of values (..., M, E) under softmax_j(-beta d_c(q_i, keys_j) + bias_ij), all at
        curvature -c, -> (..., N, E): ``gmath.hyperbolic_attention`` with k = -c, no (N, M) tensor in memory.  A fully masked query gives
        the origin."""
        from . import ball, gmath
        c = self._c("hyperbolic_attention")
        if c == 1.0:
            return gmath.hyperbolic_attention(q, keys, values, -1.0, beta, bias)
        return ball.hyperbolic_attention(c, q, keys, values, beta, bias)

    # geoopt's names
    projx = project
    transp = parallel_transport
    transp0 = parallel_transport0
    transp0back = parallel_transport0back


class Sphere:
    """Marker for unit-norm parameter rows (the reference's geoopt.manifolds.Sphere(): hyrnn_nets.py:217)."""


class ManifoldParameter(nn.Parameter):
    """The reference's geoopt.ManifoldParameter: an nn.Parameter tagged with its manifold."""

    def __new__(cls, data=None, manifold=None, requires_grad=True):
        inst = nn.Parameter.__new__(cls, data, requires_grad)
        inst.manifold = manifold
        return inst

    def __reduce_ex__(self, proto):
        return _rebuild_manifold_parameter, (self.data, self.manifold, self.requires_grad)


def _rebuild_manifold_parameter(data, manifold, requires_grad):
    return ManifoldParameter(data, manifold=manifold, requires_grad=requires_grad)


class _MobiusLinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        _check_fit("mobius_linear", x, weight, bias)
        x = _C.require_cuda(x.to(torch.float32).contiguous(), "input")
        w = _C.require_cuda(weight.contiguous(), "weight")
        b = _C.require_cuda(bias.contiguous(), "bias")
        x2 = x.reshape(-1, x.shape[-1])
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        out = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        u = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_linear_fwd(_C.ptr(x2), _C.ptr(w), _C.ptr(b), _C.ptr(out), _C.ptr(u), rows, k, n, _C.stream()),
                 "mobius_linear_fwd")
        ctx.save_for_backward(x2, w, b, u)
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], n)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, w, b, u = ctx.saved_tensors
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        go2 = go.to(torch.float32).contiguous().reshape(rows, n)
        gx = torch.empty_like(x2)
        gw = torch.empty_like(w)
        gb = torch.empty_like(b)
        nbytes = _C.lib.hypad_mobius_linear_workspace_bytes(rows, n)
        ws = torch.empty(max(nbytes // 4, 1), device=x2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_linear_bwd(_C.ptr(x2), _C.ptr(w), _C.ptr(b), _C.ptr(u), _C.ptr(go2), _C.ptr(gx), _C.ptr(gw),
                                                _C.ptr(gb), _C.ptr(ws), nbytes, rows, k, n, _C.stream()), "mobius_linear_bwd")
        return gx.view(ctx.xshape), gw, gb


def _check_fit(what, x, weight, bias=None):
    """Refuse, before any device tensor is asked for, operands whose shapes do not fit: the entry points take the sizes once and would
    read the other operand past its end."""
    if weight.dim() != 2 or x.dim() < 1 or x.shape[-1] != weight.shape[1]:
        raise _C.HypadError(f"{what}: weight must be (out_features, in_features) and the input (..., in_features), got "
                            f"{tuple(weight.shape)} and {tuple(x.shape)}")
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise _C.HypadError(f"{what}: bias must be (out_features,), got {tuple(bias.shape)} against a weight {tuple(weight.shape)}")


def _rows_of(x, weight, what, bias=None):
    _check_fit(what, x, weight, bias)
    x = _C.require_cuda(x.to(torch.float32).contiguous(), "input")
    w = _C.require_cuda(weight.contiguous(), "weight")
    return x, x.reshape(-1, x.shape[-1]), w


class _MobiusLinearExFn(torch.autograd.Function):
    """mobius_linear in any configuration (hypad_mobius_linear_ex_*).  Saved for the backward: x, the parameters and mx = x W^T."""

    @staticmethod
    def forward(ctx, x, weight, bias, flags, nonlin):
        x, x2, w = _rows_of(x, weight, "mobius_linear", bias)
        b = None if bias is None else _C.require_cuda(bias.contiguous(), "bias")
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        out = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        mx = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_linear_ex_fwd(_C.ptr(x2), _C.ptr(w), _C.ptr(b), _C.ptr(out), _C.ptr(mx), rows, k, n, flags, nonlin,
                                                   _C.stream()), "mobius_linear_ex_fwd")
        ctx.save_for_backward(x2, w, mx, *(() if b is None else (b,)))
        ctx.xshape, ctx.flags, ctx.nonlin = x.shape, flags, nonlin
        return out.view(*x.shape[:-1], n)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, w, mx, *rest = ctx.saved_tensors
        b = rest[0] if rest else None
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        go2 = go.to(torch.float32).contiguous().reshape(rows, n)
        gx = torch.empty_like(x2)
        gw = torch.empty_like(w)
        gb = None if b is None else torch.empty_like(b)
        nbytes = _C.lib.hypad_mobius_linear_ex_workspace_bytes(rows, n)
        ws = torch.empty(max(nbytes // 4, 1), device=x2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_linear_ex_bwd(_C.ptr(x2), _C.ptr(w), _C.ptr(b), _C.ptr(mx), _C.ptr(go2), _C.ptr(gx), _C.ptr(gw),
                                                   _C.ptr(gb), _C.ptr(ws), nbytes, rows, k, n, ctx.flags, ctx.nonlin, _C.stream()),
                 "mobius_linear_ex_bwd")
        return gx.view(ctx.xshape), gw, gb, None, None


class _MobiusMatvecFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, m, x):
        x, x2, w = _rows_of(x, m, "mobius_matvec")
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        out = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        mx = torch.empty(rows, n, device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_matvec_fwd(_C.ptr(x2), _C.ptr(w), _C.ptr(out), _C.ptr(mx), rows, k, n, _C.stream()),
                 "mobius_matvec_fwd")
        ctx.save_for_backward(x2, w, mx)
        ctx.xshape = x.shape
        return out.view(*x.shape[:-1], n)

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x2, w, mx = ctx.saved_tensors
        rows, k, n = x2.shape[0], x2.shape[1], w.shape[0]
        go2 = go.to(torch.float32).contiguous().reshape(rows, n)
        gx = torch.empty_like(x2)
        gw = torch.empty_like(w)
        nbytes = _C.lib.hypad_mobius_linear_ex_workspace_bytes(rows, n)
        ws = torch.empty(max(nbytes // 4, 1), device=x2.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_matvec_bwd(_C.ptr(x2), _C.ptr(w), _C.ptr(mx), _C.ptr(go2), _C.ptr(gx), _C.ptr(gw), _C.ptr(ws), nbytes,
                                                rows, k, n, _C.stream()), "mobius_matvec_bwd")
        return gw, gx.view(ctx.xshape)


_SUPPORTED = ("supported: hyperbolic_input and hyperbolic_bias True or False, bias a vector or None, nonlin None, torch.tanh, "
              "torch.relu or torch.nn.functional.relu, k = -1, fp32, a 2-D weight and dim = -1")


def _check_k(k, what):
    if abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(f"{what}: curvature k = {float(k)} is not implemented; {_SUPPORTED}")


def mobius_matvec(m, x, *, k, dim=-1):
    """M (x) x for ball-valued rows of x (reference: hyperspace/hyrnn_nets.py:38-58): one HIP launch forward, differentiable in
    m and x (first order).  A floating x of any dtype is cast to fp32; m is fp32, and so is the result."""
    _check_k(k, "mobius_matvec")
    if dim != -1 and dim != x.dim() - 1:
        raise NotImplementedError(f"mobius_matvec: dim = {dim} is not implemented; {_SUPPORTED}")
    if m.dim() != 2:
        raise NotImplementedError(f"mobius_matvec: a batched m of {m.dim()} dimensions is not implemented; {_SUPPORTED}")
    return _MobiusMatvecFn.apply(m, x)


def _nonlin_code(nonlin):
    if nonlin is None:
        return _C.NONLIN_NONE
    if nonlin is torch.tanh:
        return _C.NONLIN_TANH
    if nonlin is torch.relu or nonlin is torch.nn.functional.relu:
        return _C.NONLIN_RELU
    raise NotImplementedError(f"mobius_linear: nonlin = {nonlin!r} has no HIP kernel; {_SUPPORTED}")


def mobius_linear(input, weight, bias=None, hyperbolic_input=True, hyperbolic_bias=True, nonlin=None, k=-1.0):
    """The Moebius linear layer (reference: hyperspace/hyrnn_nets.py:13-35) on input (..., in_features): one fused HIP launch forward and
    a HIP backward in every configuration.  A floating input of any dtype is cast to fp32; weight and bias are fp32, and so is the
    result."""
    _check_k(k, "mobius_linear")
    code = _nonlin_code(nonlin)
    if weight.dim() != 2:
        raise NotImplementedError(f"mobius_linear: a batched weight of {weight.dim()} dimensions is not implemented; {_SUPPORTED}")
    if not hyperbolic_input and hyperbolic_bias and bias is not None and code == _C.NONLIN_NONE:
        return _MobiusLinearFn.apply(input, weight, bias)        # the configuration of models/tadgan.py:43-52, as before
    flags = (_C.ML_HYPER_INPUT if hyperbolic_input else 0) | (_C.ML_HYPER_BIAS if hyperbolic_bias else 0)
    return _MobiusLinearExFn.apply(input, weight, bias, flags, code)


def one_rnn_transform(W, h, U, x, b, k):
    """((W (x) h) (+) (U (x) x)) (+) b (reference: hyperspace/hyrnn_nets.py:61-65), composed from the differentiable HIP ops.  Floating
    h, x and b of any dtype are cast to fp32; W and U are fp32, and so is the result."""
    from . import gmath
    _check_k(k, "one_rnn_transform")
    return gmath.mobius_add(gmath.mobius_add(mobius_matvec(W, h, k=k), mobius_matvec(U, x, k=k), k=k), b, k=k)


_GRU_SUPPORTED = ("supported: k = -1, fp32, nonlin None, torch.tanh, torch.relu or torch.nn.functional.relu, input (steps, rows, in) -- the "
                  "cell: (rows, in) -- with a hidden state (rows, hidden), weight_ih (3 hidden, in), weight_hh (3 hidden, hidden), bias "
                  "(3, hidden), in and hidden at most 256; batch_sizes: positive, not increasing, summing to the packed rows")


class _MobiusGRUFn(torch.autograd.Function):
    """hypad_mobius_gru_*: x (steps, rows, in) and h0 (rows, hidden) on the ball -> the hidden states (steps, rows, hidden).  Saved for
    the backward: the operands, the result and the six products per (step, row)."""

    @staticmethod
    def forward(ctx, x, h0, w_ih, w_hh, bias, nonlin):
        x, h0, w_ih, w_hh, bias = (_C.require_cuda(t.to(torch.float32).contiguous(), n)
                                   for t, n in ((x, "input"), (h0, "hidden state"), (w_ih, "weight_ih"), (w_hh, "weight_hh"), (bias, "bias")))
        steps, rows, i, h = x.shape[0], x.shape[1], x.shape[2], h0.shape[1]
        out = torch.empty(steps, rows, h, device=x.device, dtype=torch.float32)
        train = any(ctx.needs_input_grad)                   # inference: nothing is saved
        saved = torch.empty(steps, rows, 6 * h, device=x.device, dtype=torch.float32) if train else None
        nbytes = _C.lib.hypad_mobius_gru_workspace_bytes(steps, rows, i, h)
        ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_gru_fwd(_C.ptr(x), _C.ptr(h0), _C.ptr(w_ih), _C.ptr(w_hh), _C.ptr(bias), _C.ptr(out), _C.ptr(saved),
                                             _C.ptr(ws), nbytes, steps, rows, i, h, nonlin, _C.stream()), "mobius_gru_fwd")
        if train:
            ctx.save_for_backward(x, h0, w_ih, w_hh, bias, out, saved)
        ctx.nonlin = nonlin
        return out

    @staticmethod
    @_C.first_order_only
    def backward(ctx, go):
        x, h0, w_ih, w_hh, bias, out, saved = ctx.saved_tensors
        steps, rows, i, h = x.shape[0], x.shape[1], x.shape[2], h0.shape[1]
        go = go.to(torch.float32).contiguous()
        grads = [torch.empty_like(t) if need else None for t, need in zip((x, h0, w_ih, w_hh, bias), ctx.needs_input_grad)]
        nbytes = _C.lib.hypad_mobius_gru_workspace_bytes(steps, rows, i, h)
        ws = torch.empty(max(nbytes // 4, 1), device=x.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_mobius_gru_bwd(_C.ptr(x), _C.ptr(h0), _C.ptr(w_ih), _C.ptr(w_hh), _C.ptr(bias), _C.ptr(out), _C.ptr(saved),
                                             _C.ptr(go), None, *(_C.ptr(g) for g in grads), _C.ptr(ws), nbytes, steps, rows, i, h, ctx.nonlin,
                                             _C.stream()), "mobius_gru_bwd")
        return (*grads, None)


def _gru_code(nonlin):
    try:
        return _nonlin_code(nonlin)
    except NotImplementedError:
        raise NotImplementedError(f"mobius_gru: nonlin = {nonlin!r} has no HIP kernel; {_GRU_SUPPORTED}") from None


def _gru_check(x, hx, weight_ih, weight_hh, bias, k, what):
    """Refuse, before any device call, what the kernels do not take.  x: (..., rows, in)."""
    if abs(float(k) + 1.0) > 1e-12:
        raise NotImplementedError(f"{what}: curvature k = {float(k)} is not implemented; {_GRU_SUPPORTED}")
    ok = (hx.dim() == 2 and weight_ih.dim() == 2 and weight_hh.dim() == 2 and x.dim() >= 2
          and weight_ih.shape == (3 * hx.shape[1], x.shape[-1]) and weight_hh.shape == (3 * hx.shape[1], hx.shape[1])
          and tuple(bias.shape) == (3, hx.shape[1]) and hx.shape[1] > 0 and x.shape[-1] > 0)
    if not ok:
        raise NotImplementedError(f"{what}: input {tuple(x.shape)}, hidden state {tuple(hx.shape)}, weight_ih {tuple(weight_ih.shape)}, weight_hh "
                                  f"{tuple(weight_hh.shape)} and bias {tuple(bias.shape)} do not fit together; {_GRU_SUPPORTED}")
    if x.shape[-1] > 256 or hx.shape[1] > 256:
        raise NotImplementedError(f"{what}: in = {x.shape[-1]}, hidden = {hx.shape[1]} is not implemented; {_GRU_SUPPORTED}")


def mobius_gru_cell(input, hx, weight_ih, weight_hh, bias, k, nonlin=None):
    """One step of the Moebius GRU (reference: hyperspace/hyrnn_nets.py:68-91): input (rows, in) and hx (rows, hidden) on the ball ->
    the next hidden state.  The sequence kernels at steps = 1: one GEMM and one launch forward, first-order differentiable.  Floating
    operands of any dtype are cast to fp32 and the result is fp32."""
    code = _gru_code(nonlin)
    _gru_check(input, hx, weight_ih, weight_hh, bias, k, "mobius_gru_cell")
    if input.dim() != 2 or input.shape[0] != hx.shape[0]:
        raise NotImplementedError(f"mobius_gru_cell: input {tuple(input.shape)} against a hidden state {tuple(hx.shape)}; {_GRU_SUPPORTED}")
    return _MobiusGRUFn.apply(input.unsqueeze(0), hx, weight_ih, weight_hh, bias, code)[0]


def mobius_gru_loop(input, h0, weight_ih, weight_hh, bias, k, batch_sizes=None, hyperbolic_input=False, hyperbolic_hidden_state0=False,
                    nonlin=None):
    """The Moebius GRU over a sequence (reference: hyperspace/hyrnn_nets.py:94-151): returns (outs, h_last).  input (steps, rows, in),
    or with ``batch_sizes`` the packed (sum(batch_sizes), in); a Euclidean input or h0 goes through expmap0 first.  Equal-length rows
    run as one autograd function on the sequence kernels (one launch for all steps, forward and backward); packed sequences run the
    reference's own slicing loop over ``mobius_gru_cell``.  Floating operands of any dtype are cast to fp32 and the results are fp32."""
    from . import gmath
    code = _gru_code(nonlin)
    _gru_check(input, h0, weight_ih, weight_hh, bias, k, "mobius_gru_loop")
    if batch_sizes is None:
        if input.dim() != 3 or input.shape[1] != h0.shape[0] or input.shape[0] < 1:
            raise NotImplementedError(f"mobius_gru_loop: input {tuple(input.shape)} against h0 {tuple(h0.shape)}; {_GRU_SUPPORTED}")
    else:
        sizes = [int(b) for b in batch_sizes]
        if (input.dim() != 2 or not sizes or sizes[0] != h0.shape[0] or min(sizes) < 1 or sum(sizes) != input.shape[0]
                or any(b > a for a, b in zip(sizes, sizes[1:]))):
            raise NotImplementedError(f"mobius_gru_loop: batch_sizes {sizes} against input {tuple(input.shape)} and h0 {tuple(h0.shape)}; "
                                      f"{_GRU_SUPPORTED}")
    hx = h0 if hyperbolic_hidden_state0 else gmath.expmap0(h0, k=k)
    if not hyperbolic_input:
        input = gmath.expmap0(input, k=k)
    if batch_sizes is None:
        outs = _MobiusGRUFn.apply(input, hx, weight_ih, weight_hh, bias, code)
        return outs, outs[-1]
    outs, h_last = [], []                                    # hyrnn_nets.py:129-150
    for t, n in enumerate(sizes):
        ix, input = input[:n], input[n:]
        hx = _MobiusGRUFn.apply(ix.unsqueeze(0), hx, weight_ih, weight_hh, bias, code)[0]
        outs.append(hx)
        if t + 1 < len(sizes):
            hx, ht = hx[:sizes[t + 1]], hx[sizes[t + 1]:]
            h_last.append(ht)
        else:
            h_last.append(hx)
    h_last.reverse()
    return torch.cat(outs), torch.cat(h_last)


def _expmap0_host(u):
    """Initialisation-time expmap0 on the host (hyrnn_nets.py:173); the run-time op is gmath.expmap0."""
    n = u.norm(dim=-1, keepdim=True).clamp_min(1e-15)
    return torch.tanh(n.clamp(-15, 15)) * (u / n)


class MobiusLinear(nn.Linear):
    """The reference's module around ``mobius_linear`` (hyperspace/hyrnn_nets.py:154-200).  As there, the input goes through ``.float()``:
    a floating input of any dtype is cast to fp32 and the result is fp32."""

    def __init__(self, *args, hyperbolic_input=True, hyperbolic_bias=True, nonlin=None, k=-1.0, fp64_hyper=True, **kwargs):
        super().__init__(*args, **kwargs)
        if fp64_hyper:
            raise NotImplementedError(f"fp64_hyper=True: the reference's hot path uses fp32 (models/tadgan.py:51); {_SUPPORTED}")
        if self.bias is not None and hyperbolic_bias:
            self.ball = PoincareBall(c=abs(float(k)))
            with torch.no_grad():
                ball_bias = _expmap0_host(self.bias.detach().clone().normal_() / 400)        # hyrnn_nets.py:173
            self.bias = ManifoldParameter(ball_bias, manifold=self.ball)
        with torch.no_grad():
            std = 1 / math.sqrt(2 * self.weight.shape[0] * self.weight.shape[1]) / 100       # hyrnn_nets.py:176-178
            self.weight.normal_(std=std)
        self.hyperbolic_bias, self.hyperbolic_input, self.nonlin = hyperbolic_bias, hyperbolic_input, nonlin
        self.k = torch.tensor(float(k))
        self.fp64_hyper = fp64_hyper

    def forward(self, input):
        return mobius_linear(input.float(), weight=self.weight, bias=self.bias, hyperbolic_input=self.hyperbolic_input,
                             nonlin=self.nonlin, hyperbolic_bias=self.hyperbolic_bias, k=float(self.k))


class MobiusDist2Hyperplane(nn.Module):
    """The hyperbolic read-out layer (reference: hyperspace/hyrnn_nets.py:210-245): the signed geodesic distance of every ball-valued
    input row to ``out_features`` hyperplanes of the ball -- through ``point`` with normal ``tangent`` -- times ``exp(scale)``; the
    counterpart of the logits of an nn.Linear.  One fused HIP launch forward and a HIP backward, ``scale`` inside the kernel.  As in the
    reference, the input goes through ``.float()``: a floating input of any dtype is cast to fp32 and the result is fp32.

    Curvature: k = -1, the Poincare ball.  The reference's module passes ``k=self.ball.c`` = +1 to dist2plane, a call written for an
    older geoopt whose argument was ``c``; with the vendored math_.py that selects the spherical formulas, which is not what a layer
    of the ball means.  This layer computes k = -1 and accepts no other k.

    ``point`` and ``tangent`` are tagged ManifoldParameters (ball / Sphere), as in the reference, so that a Riemannian optimiser moves
    them on their manifolds: ``hypad_amd.optim.RiemannianAdam(layer.parameters(), manifold_rows=True)`` and
    ``hypad_amd.optim.RiemannianSGD`` update every row of ``point`` as a point of the ball and every row of ``tangent`` as a unit
    vector, one launch per parameter and step (docs/history/riemannian_rows.md).  Without ``manifold_rows`` RiemannianAdam refuses
    the two, as it always did; Euclidean optimisers (torch.optim.SGD / Adam) train the layer as well, off the manifolds.
    """

    def __init__(self, in_features, out_features, k=-1.0, fp64_hyper=False):
        super().__init__()
        _check_k(k, "MobiusDist2Hyperplane")
        if fp64_hyper:
            raise NotImplementedError(f"fp64_hyper=True: the HIP kernels are fp32; {_SUPPORTED}")
        self.in_features, self.out_features, self.fp64_hyper = in_features, out_features, fp64_hyper
        self.ball, self.sphere = PoincareBall(c=abs(float(k))), Sphere()
        self.scale = nn.Parameter(torch.zeros(out_features))
        point = _expmap0_host(torch.randn(out_features, in_features) / 4)                # hyrnn_nets.py:219-220
        tangent = torch.randn(out_features, in_features)
        tangent = tangent / tangent.norm(dim=-1, keepdim=True)                           # Sphere.proj_ (:225)
        self.point = ManifoldParameter(point, manifold=self.ball)
        self.tangent = ManifoldParameter(tangent, manifold=self.sphere)

    def forward(self, input):
        from .gmath import _Dist2Plane
        return _Dist2Plane.apply(input.float(), self.point, self.tangent, self.scale, _C.D2P_SIGNED)

    def extra_repr(self):
        return f"in_features={self.in_features}, out_features={self.out_features}"
