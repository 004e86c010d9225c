"""The row-wise Riemannian optimiser steps restated in plain torch for any dtype: geoopt 0.5.0's RiemannianAdam.step and
RiemannianSGD.step (with Manifold.retr_transp, Manifold.component_inner and Sphere) for parameters whose rows are points of the Poincare
ball at k = -1 or unit vectors, and SGD's rule on plain rows.  geoopt is neither installed nor in the reference tree: the rules are the
specification (docs/history/riemannian_rows.md).  tests/test_riemann_opt_host.py ties the ball / Adam branch to the pinned
oracle/manual.radam_ball_step and oracle/radam.RiemannianAdam; tests/test_gpu_riemann_opt.py uses these functions in fp64 as the
reference and in fp32 as the yardstick of the kernels of csrc/riemann_opt.hip.

Everything is (rows, D): a row is one point, its gradient row and its state rows.  ``t`` is the step number, ``stabilize`` None / 0 for
never.  Functions return new tensors and change none of their arguments.
"""
import torch

from oracle import gmath

EPS = 1e-15                       # the floor under the sphere's norm (this library's; geoopt divides unguarded)


class BallRows:
    """PoincareBall at k = -1 out of oracle/gmath (math_.py's functions); project at the fp32 limit 1 - 4e-3 in every dtype, the limit of
    the fp32 parameters the kernels update (as oracle/manual.radam_ball_step's maxnorm)."""

    @staticmethod
    def rgrad(x, g):
        return gmath.egrad2rgrad(x, g)

    @staticmethod
    def inner(x, r):
        return gmath.inner(x, r, r, keepdim=True)

    @staticmethod
    def retr(x, u):
        return gmath.project(x + u, eps=gmath.PROJ_EPS_F32)

    @staticmethod
    def transp(x, y, w):
        return gmath.parallel_transport(x, y, w)

    @staticmethod
    def stabilise(x, w):
        return gmath.project(x, eps=gmath.PROJ_EPS_F32), w


def _dot(a, b):
    return (a * b).sum(-1, keepdim=True)


class SphereRows:
    @staticmethod
    def rgrad(x, g):
        return g - _dot(x, g) * x

    @staticmethod
    def inner(x, r):
        return _dot(r, r)

    @staticmethod
    def retr(x, u):
        y = x + u
        return y / y.norm(dim=-1, keepdim=True).clamp_min(EPS)

    @staticmethod
    def transp(x, y, w):
        return w - _dot(y, w) * y

    @staticmethod
    def stabilise(x, w):
        x = x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)
        return x, w - _dot(x, w) * x


class EuclideanRows:
    rgrad = staticmethod(lambda x, g: g)
    retr = staticmethod(lambda x, u: x + u)
    transp = staticmethod(lambda x, y, w: w)
    stabilise = staticmethod(lambda x, w: (x, w))


def _stabilises(t, stabilize):
    return bool(stabilize) and t % stabilize == 0


def radam_rows(man, x, g, m, v, t, lr, b1, b2, eps, wd=0.0, stabilize=None):
    """One RiemannianAdam step of every row -> (x, exp_avg, exp_avg_sq)."""
    g = g + wd * x
    r = man.rgrad(x, g)
    m = b1 * m + (1 - b1) * r
    v = b2 * v + (1 - b2) * man.inner(x, r)                      # one number per row, on every element of the row
    direction = (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
    y = man.retr(x, -lr * direction)
    m = man.transp(x, y, m)
    if _stabilises(t, stabilize):
        y, m = man.stabilise(y, m)
    return y, m, v


def rsgd_rows(man, x, g, buf, t, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, stabilize=None):
    """One RiemannianSGD step of every row -> (x, momentum_buffer); buf is None exactly where momentum == 0.  (A parameter's first step
    with momentum starts from buf = a clone of the incoming g: the optimiser class does that, and so does ``rsgd_run``.)"""
    g = g + wd * x
    r = man.rgrad(x, g)
    if momentum == 0:
        assert buf is None
        y = man.retr(x, -lr * r)
        if _stabilises(t, stabilize):
            y = man.stabilise(y, torch.zeros_like(y))[0]
        return y, None
    buf = momentum * buf + (1 - dampening) * r
    d = r + momentum * buf if nesterov else buf
    y = man.retr(x, -lr * d)
    buf = man.transp(x, y, buf)
    if _stabilises(t, stabilize):
        y, buf = man.stabilise(y, buf)
    return y, buf


def radam_ball_rows(x, g, m, v, t, lr, b1, b2, eps, wd=0.0, stabilize=None):
    return radam_rows(BallRows, x, g, m, v, t, lr, b1, b2, eps, wd, stabilize)


def radam_sphere_rows(x, g, m, v, t, lr, b1, b2, eps, wd=0.0, stabilize=None):
    return radam_rows(SphereRows, x, g, m, v, t, lr, b1, b2, eps, wd, stabilize)


def rsgd_ball_rows(x, g, buf, t, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, stabilize=None):
    return rsgd_rows(BallRows, x, g, buf, t, lr, momentum, dampening, wd, nesterov, stabilize)


def rsgd_sphere_rows(x, g, buf, t, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, stabilize=None):
    return rsgd_rows(SphereRows, x, g, buf, t, lr, momentum, dampening, wd, nesterov, stabilize)


def rsgd_euclidean_rows(x, g, buf, t, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, stabilize=None):
    return rsgd_rows(EuclideanRows, x, g, buf, t, lr, momentum, dampening, wd, nesterov, stabilize)


MANIFOLDS = {"ball": BallRows, "sphere": SphereRows, "euclidean": EuclideanRows}


def radam_run(man, x, grads, lr, b1, b2, eps, wd=0.0, stabilize=None):
    """The optimiser class's trajectory from fresh state over the recorded gradients -> [(x, exp_avg, exp_avg_sq) after every step]."""
    m, v, out = torch.zeros_like(x), torch.zeros_like(x), []
    for t, g in enumerate(grads, 1):
        x, m, v = radam_rows(man, x, g.to(x.dtype), m, v, t, lr, b1, b2, eps, wd, stabilize)
        out.append((x, m, v))
    return out


def rsgd_run(man, x, grads, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, stabilize=None):
    """-> [(x, momentum_buffer or None) after every step]; with momentum the buffer starts as the first gradient itself."""
    buf, out = None, []
    for t, g in enumerate(grads, 1):
        g = g.to(x.dtype)
        if momentum != 0 and buf is None:
            buf = g.clone()
        x, buf = rsgd_rows(man, x, g, buf, t, lr, momentum, dampening, wd, nesterov, stabilize)
        out.append((x, buf))
    return out
