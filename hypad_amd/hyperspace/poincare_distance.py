"""Pair-wise Poincare distance (reference: hyperspace/poincare_distance.py:5-16) as one MFMA kernel."""
import torch

from .. import _C


def poincare_distance(pred, gt):
    """(N, D), (M, D) -> (N, M): acosh(1 + 2 clamp(|x-y|^2, 1e-7) / ((1-clamp(|x|^2,1e-5))(1-clamp(|y|^2,1e-5)))).

    Forward only: the kernel has no backward, so an operand that requires grad while autograd is recording is refused -- the result would
    carry no graph, and a loss built on it would train nothing without an error.  The differentiable pair-wise distance is
    ``gmath.dist_matmul``.  Floating operands of any dtype are cast to fp32 and the result is fp32."""
    if torch.is_grad_enabled() and (pred.requires_grad or gt.requires_grad):
        raise _C.HypadError("poincare_distance is forward only and its result carries no graph: call it under torch.no_grad() or on detached "
                            "operands; the differentiable pair-wise distance is gmath.dist_matmul")
    if pred.dim() != 2 or gt.dim() != 2 or pred.shape[1] != gt.shape[1]:
        raise _C.HypadError(f"poincare_distance: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must be (N, D) and (M, D)")
    pred = _C.require_cuda(pred.to(torch.float32).contiguous(), "pred")
    gt = _C.require_cuda(gt.to(torch.float32).contiguous(), "gt")
    (n, d), m = pred.shape, gt.shape[0]
    out = torch.empty(n, m, device=pred.device, dtype=torch.float32)
    if n and m:                                              # (no pairs: nothing to launch; an empty operand's data pointer is null)
        _C.check(_C.lib.hypad_poincare_pairdist_fwd(_C.ptr(pred), _C.ptr(gt), _C.ptr(out), n, m, d, _C.stream()), "pairdist")
    return out
