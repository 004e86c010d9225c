"""Optimizers of the hot path as stand-alone HIP steps.

``Adam`` follows ``torch.optim.Adam`` (train.py:274-281); ``RiemannianAdam`` restates
``geoopt.optim.RiemannianAdam`` (train.py:282-288; geoopt==0.5.0 -- not vendored in the reference, see
oracle/radam.py for the rule and its pinning status).  Inside the fused training iterations the same update
runs in the epilogue of the weight-gradient kernel; these classes exist for callers that bring their own
``.grad`` tensors, and to carry hyper-parameters / state for ``hypad_amd.train``.

Row-wise Riemannian steps (csrc/riemann_opt.hip, docs/history/riemannian_rows.md): a tagged parameter whose rows are points of the
Poincare ball (c = 1) or unit vectors (Sphere) -- MobiusDist2Hyperplane's ``point`` and ``tangent`` -- is updated row by row on its
manifold, one launch per parameter and step, by ``RiemannianAdam(..., manifold_rows=True)`` and by ``RiemannianSGD``.  Without the
keyword RiemannianAdam updates what it always did, 1-D ball vectors and untagged parameters, and refuses the rest.  The rules restate
geoopt 0.5.0's ``RiemannianAdam.step`` / ``RiemannianSGD.step``; geoopt is not at hand to compare against, so parity with geoopt itself
is unpinned for the Sphere branch and for RiemannianSGD (the ball branch of Adam reduces to what oracle/radam.py pins).  Two places
are this library's own: the sphere's norm is floored at 1e-15 where geoopt divides unguarded, and a row of ``exp_avg_sq`` that holds
one value repeated keeps holding one value repeated, bit for bit.  State keys are geoopt's (``step``, ``exp_avg``, ``exp_avg_sq``,
``momentum_buffer``), so the optimiser state of a geoopt checkpoint loads.

A step takes its step number by value, so a step captured into a graph would replay the same bias correction for ever: run the steps
eagerly (on any stream; they go to torch's current one), and capture only what comes before them.
"""
import torch

from . import _C

MAX_ROW_DIM = 256                # csrc/riemann_opt.hip: a row per wave, 64 lanes x 4 elements


def _is_ball(p):
    return getattr(p, "manifold", None) is not None


def _check_ball_vector(p):
    """The Riemannian step (hypad_radam_step) updates a tagged parameter as ONE point of the ball with numel coordinates.  That is
    right for the 1-D ball biases of MobiusLinear and wrong for anything else -- MobiusDist2Hyperplane's ``point`` is out_features
    points, its ``tangent`` lies on a sphere -- so anything else is refused, not silently updated as one vector."""
    if not _is_ball(p):
        return
    from .hyperspace.hyrnn_nets import PoincareBall
    if p.dim() != 1 or not isinstance(p.manifold, PoincareBall):
        raise NotImplementedError(f"RiemannianAdam: a {type(p.manifold).__name__} parameter of shape {tuple(p.shape)} has no Riemannian update "
                                  "yet (supported: 1-D PoincareBall vectors); train MobiusDist2Hyperplane's point / tangent with a "
                                  "Euclidean optimiser (torch.optim.SGD / Adam, hypad_amd.optim.Adam), or pass manifold_rows=True for the "
                                  "row-wise Riemannian step")


def _is_ball_vector(p):
    from .hyperspace.hyrnn_nets import PoincareBall
    return p.dim() == 1 and isinstance(getattr(p, "manifold", None), PoincareBall)


def _manifold_rows(p, who):
    """How a tagged parameter goes through the row-wise steps: (HYPAD_MANIFOLD_*, rows, dim), every slice along the last dimension one
    point of its manifold; None for an untagged parameter.  Whatever the kernels do not cover is refused here, before any device call."""
    man = getattr(p, "manifold", None)
    if man is None:
        return None
    from .hyperspace.hyrnn_nets import PoincareBall, Sphere
    what = f"{who}: a {type(man).__name__} parameter of shape {tuple(p.shape)}"
    if isinstance(man, PoincareBall):
        if float(man.c) != 1.0:
            raise NotImplementedError(f"{what} with c = {float(man.c):g} has no row-wise Riemannian update (supported: c = 1, the ball at k = -1)")
        kind = _C.MANIFOLD_BALL
    elif isinstance(man, Sphere):
        kind = _C.MANIFOLD_SPHERE
    else:
        raise NotImplementedError(f"{what} has no row-wise Riemannian update (supported: PoincareBall at c = 1 and Sphere)")
    if p.dim() < 1 or p.shape[-1] > MAX_ROW_DIM:
        raise NotImplementedError(f"{what} has no row-wise Riemannian update (supported: a last dimension from 1 to {MAX_ROW_DIM})")
    if not p.is_contiguous():
        raise NotImplementedError(f"{what} is not contiguous (supported: contiguous parameters; the step updates the rows in place)")
    dim = p.shape[-1]
    return kind, p.numel() // max(dim, 1), dim


def _euclidean_rows(n):
    """An untagged parameter of n elements for the row-wise SGD step: its rule is elementwise, so any split into rows gives the same
    bits; the widest row that divides n keeps the lanes busy."""
    dim = next(d for d in range(min(MAX_ROW_DIM, max(n, 1)), 0, -1) if n % d == 0)
    return _C.MANIFOLD_EUCLIDEAN, n // dim, dim


class _Base(torch.optim.Optimizer):
    riemannian = False

    def _state(self, p):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = 0
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            group["step"] = group.get("step", 0) + 1
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                rows = None
                if self.riemannian:
                    # manifold_rows: tagged parameters row by row on their manifold; a 1-D ball vector keeps the step it always had
                    if group.get("manifold_rows") and not _is_ball_vector(p):
                        rows = _manifold_rows(p, "RiemannianAdam")
                    else:
                        _check_ball_vector(p)
                _C.require_cuda(p.data, "parameter")
                g = _C.require_cuda(p.grad.contiguous(), "gradient")
                st = self._state(p)
                st["step"] = group["step"]
                n = p.numel()
                if rows is not None:
                    rc = _C.lib.hypad_radam_rows_step(_C.ptr(p.data), _C.ptr(g), _C.ptr(st["exp_avg"]), _C.ptr(st["exp_avg_sq"]), rows[1], rows[2],
                                                      rows[0], group["step"], group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                                      int(group.get("stabilize") or 0), _C.stream())
                elif self.riemannian:
                    ball = n if _is_ball(p) else 0
                    rc = _C.lib.hypad_radam_step(_C.ptr(p.data), _C.ptr(g), _C.ptr(st["exp_avg"]), _C.ptr(st["exp_avg_sq"]), n, 0,
                                                 ball, group["step"], group["lr"], b1, b2, group["eps"], group["weight_decay"],
                                                 int(group.get("stabilize") or 0), _C.stream())
                else:
                    rc = _C.lib.hypad_adam_step(_C.ptr(p.data), _C.ptr(g), _C.ptr(st["exp_avg"]), _C.ptr(st["exp_avg_sq"]), n,
                                                group["step"], group["lr"], b1, b2, group["eps"], group["weight_decay"], _C.stream())
                _C.check(rc, type(self).__name__ + ".step")
        return loss


class Adam(_Base):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))


class RiemannianAdam(_Base):
    """``manifold_rows`` (per group, default off): a PoincareBall (c = 1) or Sphere parameter of rank >= 2, or a rank-1 Sphere vector, is
    updated row by row on its manifold -- every slice along the last dimension (at most 256 long) one point -- by one launch of
    hypad_radam_rows_step per step.  1-D ball vectors and untagged parameters keep their steps, bit for bit.  Off, such parameters are
    refused as before.  The sphere's retraction and stabilisation divide by max(|x|, 1e-15) where geoopt divides by |x|."""
    riemannian = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stabilize=None, manifold_rows=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, stabilize=stabilize, manifold_rows=manifold_rows))


class RiemannianSGD(torch.optim.Optimizer):
    """geoopt.optim.RiemannianSGD restated (geoopt 0.5.0; parity with geoopt itself is unpinned), one launch of hypad_rsgd_rows_step per
    parameter and step.  A PoincareBall (c = 1) or Sphere parameter is updated row by row on its manifold, every slice along the last
    dimension (at most 256 long) one point and a rank-1 parameter one row; an untagged parameter takes the same rule with identity maps.
    With momentum, the buffer of a parameter's first step is a clone of the incoming Euclidean gradient, taken before weight decay and
    before the Riemannian gradient -- geoopt's own behaviour, kept.  The sphere's retraction and stabilisation divide by
    max(|x|, 1e-15) where geoopt divides by |x|.  A step takes its number by value and runs eagerly on torch's current stream: it is
    not meant for graph capture."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, stabilize=None):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      stabilize=stabilize))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            group["step"] = group.get("step", 0) + 1
            for p in group["params"]:
                if p.grad is None or p.numel() == 0:
                    continue
                kind, rows, dim = _manifold_rows(p, "RiemannianSGD") or _euclidean_rows(p.numel())
                _C.require_cuda(p.data, "parameter")
                g = _C.require_cuda(p.grad.contiguous(), "gradient")
                st = self.state[p]
                st["step"] = group["step"]
                buf = None
                if group["momentum"] != 0:
                    if "momentum_buffer" not in st:
                        st["momentum_buffer"] = g.clone(memory_format=torch.contiguous_format)
                    buf = _C.require_cuda(st["momentum_buffer"], "momentum_buffer")
                rc = _C.lib.hypad_rsgd_rows_step(_C.ptr(p.data), _C.ptr(g), _C.ptr(buf), rows, dim, kind, group["step"], group["lr"],
                                                 group["momentum"], group["dampening"], group["weight_decay"], int(bool(group["nesterov"])),
                                                 int(group.get("stabilize") or 0), _C.stream())
                _C.check(rc, "RiemannianSGD.step")
        return loss
