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

By default a step takes its step number by value and launches once per parameter, so a step captured into a graph would replay the
same bias correction for ever: such steps run eagerly (on any stream; they go to torch's current one), and only what comes before them
is captured.

``capturable=True`` (per group, on all three classes; csrc/optim_group.hip, docs/history/capturable_optim.md) makes the whole step
capturable: ``group["step"]`` becomes a one-element int32 CUDA tensor that every ``state[p]["step"]`` refers to, a step is one launch that
adds one to it and one grouped launch per 32 parameters that reads it, and nothing is read back to the host.  ``group["lr"]`` may then be
a one-element fp32 CUDA tensor, so that a schedule can drive a captured step.  Tagged parameters go row by row on their manifold as
above; an untagged tensor takes torch.optim.Adam's element-wise rule (or SGD's) in rows of 256 elements; a 1-D ball vector of at most
256 elements goes through as one ball row.  State is created only outside a capture: run one eager step, then capture
zero_grad / forward / backward / step as one graph.  With ``capturable`` off, every class runs the launches and the bits it always did.
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


def _plain_rows(n):
    """An untagged tensor of n elements for the grouped steps: rows of 256 elements and a short last row (no divisor is looked for: a
    tensor of prime length would go one element per wave)."""
    return _C.MANIFOLD_EUCLIDEAN, -(-n // MAX_ROW_DIM), MAX_ROW_DIM


def _step_to_mode(step, capturable, device=None):
    """A step count as an optimiser of the given mode keeps it: a one-element int32 tensor on ``device`` when capturable (and a device
    is known), else an int.  Takes an int or a one-element tensor of any dtype and device; reading a tensor synchronises, which is why
    this runs in load_state_dict and never in step()."""
    n = int(step.item()) if isinstance(step, torch.Tensor) else int(step)
    if capturable and device is not None:
        return torch.full((1,), n, dtype=torch.int32, device=device)
    return n


def _refuse_tensor_lr(group, who):
    if isinstance(group["lr"], torch.Tensor):
        raise TypeError(f"{who}: lr is a tensor, which only a capturable step reads (the default step takes lr by value): pass "
                        "capturable=True, or a float")


def _grouped_step(opt, group, kind_of, sgd):
    """One capturable step of a group: hypad_optim_step_advance on the group's device counter, then one grouped launch per 32 of its
    parameters that have a gradient.  Everything that can be refused is refused before the first device call, and nothing is read back."""
    who = type(opt).__name__
    plan = [(p, kind_of(p)) for p in group["params"] if p.grad is not None and p.numel() > 0]
    grads = []
    for p, _ in plan:
        _C.require_cuda(p.data, "parameter")
        grads.append(_C.require_cuda(p.grad.contiguous(), "gradient"))
    lr = group["lr"]
    if isinstance(lr, torch.Tensor):
        if lr.numel() != 1:
            raise _C.HypadError(f"{who}: lr as a tensor must hold one element, got {tuple(lr.shape)}")
        _C.require_cuda(lr, "lr")
    counter = group.get("step", 0)
    if not plan and not isinstance(counter, torch.Tensor):             # (nothing to launch and no device to count on yet)
        group["step"] = counter + 1
        return
    keys = (("momentum_buffer",) if group["momentum"] != 0 else ()) if sgd else ("exp_avg", "exp_avg_sq")
    fresh = not isinstance(counter, torch.Tensor) or any(k not in opt.state[p] for p, _ in plan for k in keys)
    if fresh and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{who}: the step counter or a parameter's state does not exist yet, and creating it here would bake its "
                           "initial values into the graph: run one eager step before capturing")
    if not isinstance(counter, torch.Tensor):
        counter = group["step"] = _step_to_mode(counter, True, plan[0][0].device)
    for (p, _), g in zip(plan, grads):
        st = opt.state[p]
        st["step"] = counter
        for k in keys:
            if k not in st:
                # (RiemannianSGD: the buffer starts as a clone of the incoming Euclidean gradient, as in the default step)
                st[k] = g.clone(memory_format=torch.contiguous_format) if sgd else torch.zeros_like(p, memory_format=torch.contiguous_format)
            if _C.require_cuda(st[k], k).numel() != p.numel():
                raise _C.HypadError(f"{who}: {k} holds {st[k].numel()} elements, its parameter {p.numel()}")
    _C.require_cuda(counter, "step", torch.int32)
    stream = _C.stream()
    _C.check(_C.lib.hypad_optim_step_advance(_C.ptr(counter), stream), who + ".step")
    lr_dev, lr_val = (_C.ptr(lr), 0.0) if isinstance(lr, torch.Tensor) else (None, lr)
    stabilize = int(group.get("stabilize") or 0)
    for lo in range(0, len(plan), _C.OPTIM_GROUP_MAX):
        part = plan[lo:lo + _C.OPTIM_GROUP_MAX]
        descs = (_C.OptimTensor * len(part))()
        for d, (p, (kind, rows, dim)), g in zip(descs, part, grads[lo:]):
            st = opt.state[p]
            d.param, d.grad, d.rows, d.numel, d.dim, d.manifold = p.data_ptr(), g.data_ptr(), rows, p.numel(), dim, kind
            if keys:
                d.state0 = st[keys[0]].data_ptr()
            if len(keys) == 2:
                d.state1 = st[keys[1]].data_ptr()
        if sgd:
            rc = _C.lib.hypad_optim_group_sgd(descs, len(part), _C.ptr(counter), 0, lr_dev, lr_val, group["momentum"], group["dampening"],
                                              group["weight_decay"], int(bool(group["nesterov"])), stabilize, stream)
        else:
            b1, b2 = group["betas"]
            rc = _C.lib.hypad_optim_group_adam(descs, len(part), _C.ptr(counter), 0, lr_dev, lr_val, b1, b2, group["eps"],
                                               group["weight_decay"], stabilize, stream)
        _C.check(rc, who + ".step")


class _StepModes:
    """state_dict / load_state_dict of an optimiser whose groups count their steps as an int (default) or as a device tensor
    (capturable).  A saved ``step`` of either kind loads into either mode: it is converted here, at load time, to the mode this
    optimiser was built with (the saved group's ``capturable`` does not replace it), and the per-parameter ``step`` entries are tied to
    their group's counter again."""

    def load_state_dict(self, state_dict):
        modes = [bool(g.get("capturable", False)) for g in self.param_groups]
        as_int = lambda st: {k: (_step_to_mode(v, False) if k == "step" else v) for k, v in st.items()}
        sd = dict(state_dict)
        sd["param_groups"] = [as_int(g) for g in state_dict["param_groups"]]
        sd["state"] = {k: as_int(st) for k, st in state_dict["state"].items()}
        super().load_state_dict(sd)
        for group, capturable in zip(self.param_groups, modes):
            group["capturable"] = capturable
            dev = next((p.device for p in group["params"] if p.is_cuda), None)
            group["step"] = _step_to_mode(group.get("step", 0), capturable, dev)
            for p in group["params"]:
                if "step" in self.state.get(p, {}):
                    self.state[p]["step"] = group["step"]


class _Base(_StepModes, torch.optim.Optimizer):
    riemannian = False

    def _kind(self, group, p):
        """How a parameter goes through the grouped step: (HYPAD_MANIFOLD_*, rows, dim); the refusals of the default step, before any
        device call."""
        if not self.riemannian:
            return _plain_rows(p.numel())
        if _is_ball_vector(p):                       # one ball row; longer than a row holds: refused with the supported range
            return _manifold_rows(p, "RiemannianAdam")
        if group.get("manifold_rows"):
            return _manifold_rows(p, "RiemannianAdam") or _plain_rows(p.numel())
        _check_ball_vector(p)
        return _plain_rows(p.numel())

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
            if group.get("capturable"):
                _grouped_step(self, group, lambda p: self._kind(group, p), sgd=False)
                continue
            _refuse_tensor_lr(group, type(self).__name__)
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
    """``capturable`` (per group, default off): the step counter lives on the device and a step is one grouped launch per 32 parameters
    (the module docstring): forward, backward and step can be captured as one graph after one eager step."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, capturable=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, capturable=capturable))


class RiemannianAdam(_Base):
    """``manifold_rows`` (per group, default off): a PoincareBall (c = 1) or Sphere parameter of rank >= 2, or a rank-1 Sphere vector, is
    updated row by row on its manifold -- every slice along the last dimension (at most 256 long) one point -- by one launch of
    hypad_radam_rows_step per step.  1-D ball vectors and untagged parameters keep their steps, bit for bit.  Off, such parameters are
    refused as before.  The sphere's retraction and stabilisation divide by max(|x|, 1e-15) where geoopt divides by |x|.

    ``capturable`` (per group, default off): the step counter lives on the device and a step is one grouped launch per 32 parameters
    (hypad_optim_group_adam), so that forward, backward and step can be captured as one graph after one eager step.  Tagged parameters
    still need ``manifold_rows=True``; a 1-D ball vector goes through as one ball row and may then hold at most 256 elements; untagged
    tensors take torch.optim.Adam's element-wise rule."""
    riemannian = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, stabilize=None, manifold_rows=False, capturable=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, stabilize=stabilize, manifold_rows=manifold_rows,
                                      capturable=capturable))


class RiemannianSGD(_StepModes, torch.optim.Optimizer):
    """geoopt.optim.RiemannianSGD restated (geoopt 0.5.0; parity with geoopt itself is unpinned), one launch of hypad_rsgd_rows_step per
    parameter and step.  A PoincareBall (c = 1) or Sphere parameter is updated row by row on its manifold, every slice along the last
    dimension (at most 256 long) one point and a rank-1 parameter one row; an untagged parameter takes the same rule with identity maps.
    With momentum, the buffer of a parameter's first step is a clone of the incoming Euclidean gradient, taken before weight decay and
    before the Riemannian gradient -- geoopt's own behaviour, kept.  The sphere's retraction and stabilisation divide by
    max(|x|, 1e-15) where geoopt divides by |x|.  By default a step takes its number by value and runs eagerly on torch's current
    stream: it is not meant for graph capture.

    ``capturable`` (per group, default off): the step counter lives on the device and a step is one grouped launch per 32 parameters
    (hypad_optim_group_sgd), so that forward, backward and step can be captured as one graph after one eager step -- the step in which
    the momentum buffers are cloned from the first gradients."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, stabilize=None, capturable=False):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                                      stabilize=stabilize, capturable=capturable))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if group.get("capturable"):
                _grouped_step(self, group, lambda p: _manifold_rows(p, "RiemannianSGD") or _plain_rows(p.numel()), sgd=True)
                continue
            _refuse_tensor_lr(group, "RiemannianSGD")
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
