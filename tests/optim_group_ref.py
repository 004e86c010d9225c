"""The element-wise Adam rule of the grouped optimiser step (csrc/optim_group.hip, HYPAD_MANIFOLD_EUCLIDEAN under hypad_optim_group_adam)
restated in plain torch for any dtype, and one grouped step of a mixed list of tensors assembled from it and from the row-wise rules of
tests/riemann_opt_ref.py, which this file imports unchanged.  tests/test_optim_capturable_host.py ties ``adam_elementwise`` to
torch.optim.Adam; tests/test_gpu_optim_capturable.py uses ``group_step`` in fp64 as the reference and in fp32 as the yardstick.
"""
import riemann_opt_ref as ref


def adam_elementwise(x, g, m, v, t, lr, b1, b2, eps, wd=0.0):
    """One torch.optim.Adam step of every element -> (x, exp_avg, exp_avg_sq)."""
    g = g + wd * x
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    x = x - lr * (m / (1 - b1 ** t)) / ((v / (1 - b2 ** t)).sqrt() + eps)
    return x, m, v


def group_step(rule, tensors, t, lr, hp, wd=0.0, stabilize=None, dtype=None):
    """One grouped step.  tensors: [(manifold name, x, g, states)] with states (m, v) under "adam" and (buf,) or () under "sgd"; a
    manifold's tensors are (rows, D), a plain ("euclidean") one has any shape.  hp: (b1, b2, eps) for Adam, (momentum, dampening,
    nesterov) for SGD.  -> [(x, *states)] in ``dtype`` (default: as given)."""
    out = []
    for man, x, g, st in tensors:
        if dtype is not None:
            x, g, st = x.to(dtype), g.to(dtype), [s.to(dtype) for s in st]
        if rule == "adam":
            b1, b2, eps = hp
            if man == "euclidean":
                out.append(adam_elementwise(x, g, st[0], st[1], t, lr, b1, b2, eps, wd))
            else:
                out.append(ref.radam_rows(ref.MANIFOLDS[man], x, g, st[0], st[1], t, lr, b1, b2, eps, wd, stabilize))
        else:
            mu, damp, nest = hp
            y, b = ref.rsgd_rows(ref.MANIFOLDS[man], x, g, st[0] if st else None, t, lr, mu, damp, wd, nest, stabilize)
            out.append((y,) if b is None else (y, b))
    return out
