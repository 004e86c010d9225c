"""The stand-alone optimizer steps (csrc/ops_dense.hip: hypad_adam_step, hypad_radam_step; the rules are adam_update and
radam_ball_wave of csrc/train_common.h, the code the training kernels run) against oracle/manual.py's adam_step, radam_euclid_step
and radam_ball_step in fp64, one step at a time.

What is compared, all under ``sweep_common.Checker.cmp`` (errgpu <= C * err32 + F, err32 from the same oracle rule run in fp32 on the
CPU): exp_avg, exp_avg_sq, and the parameter as the STEP (p_new - p_old) / lr -- comparing p_new itself lets a wrong step hide under
max(1, |p|).  lr = 0.05 and |p| <= 0.1 in the Euclidean runs: the fp32 rounding of p is then below 2e-7 of the step.  One run at
the shipped hyper-parameters (lr 5e-4, weight decay 1e-5) stays under the plain rule on p_new.

Data.  Gradient magnitudes log-uniform in [1e-6, 1] with random signs.  Moments: m ~ 0.1 N(0, 1), v = m^2 + U(0, 0.01), so that a
step started at any count shows weight decay and bias correction; every fifth element starts from m = v = 0 instead: there the
denominator is sqrt(v-hat) + eps with sqrt(v-hat) down to |g| = 1e-6, the regime where eps (1e-8) and its place relative to the
bias correction decide up to a hundredth of the step.  On those elements p takes the sign of g, so that g + wd * p cannot cancel and
the sign of the step is that of an input.
"""
import numpy as np
import pytest
import torch

from oracle import manual
from sweep_common import SENTINEL, Ck, _at_offset

pytestmark = pytest.mark.gpu

F64, F32 = torch.float64, torch.float32
HYPAD_OK, HYPAD_EINVAL = 0, -1                       # include/hypad.h
f32 = lambda x: float(np.float32(x))
# The entry points take their hyper-parameters as C floats, so the operation under test is the rule AT those floats: the reference gets
# the same numbers.  (Fed 0.999 where the kernel gets 0.999f = 0.999 + 1.3e-8, the fp64 rule itself moves by 2.6e-6 of the step at
# step 1000 -- 1 - beta2^1000 changes by 7.5e-6 -- and the comparison would measure that, not the kernel.)
LR, B1, B2, EPS = f32(0.05), f32(0.9), f32(0.999), f32(1e-8)
GRID_EDGE = 2048 * 256                               # elements one pass of adam_flat_kernel's grid covers
STEPS, WDS = (1, 2, 10, 1000), (0.0, f32(0.1))


def _C():
    from hypad_amd import _C as c
    return c


def _finish(cks, what):
    print(f"\noptimizer sweep {what}: worst errgpu / allowance {max(ck.worst for ck in cks):.3f} over {len(cks)} cases")
    failures = []
    for ck in cks:
        failures += ck.failures
    assert not failures, "\n".join(failures)


def _euclid_data(g, n):
    p = torch.rand(n, generator=g) * 0.2 - 0.1
    mag = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 6 - 6)
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    grad = (mag * sign).float()
    m = 0.1 * torch.randn(n, generator=g)
    v = m * m + 0.01 * torch.rand(n, generator=g)
    fresh = torch.arange(n) % 5 == 0
    m[fresh], v[fresh] = 0.0, 0.0
    p[fresh] = p[fresh].abs() * torch.sign(grad[fresh])
    return p, grad, m, v


def _gpu_adam(p, g, m, v, step, lr, wd, dev=lambda t: t.cuda()):
    c = _C()
    P, G, M, V = (dev(t) for t in (p, g, m, v))
    c.check(c.lib.hypad_adam_step(c.ptr(P), c.ptr(G), c.ptr(M), c.ptr(V), p.numel(), step, lr, B1, B2, EPS, wd, c.stream()), "adam_step")
    torch.cuda.synchronize()
    return P.cpu(), M.cpu(), V.cpu()


def _gpu_radam(p, g, m, v, off, dim, step, lr, wd, stabilize):
    c = _C()
    P, G, M, V = (t.cuda() for t in (p, g, m, v))
    c.check(c.lib.hypad_radam_step(c.ptr(P), c.ptr(G), c.ptr(M), c.ptr(V), p.numel(), off, dim, step, lr, B1, B2, EPS, wd, stabilize, c.stream()),
            "radam_step")
    torch.cuda.synchronize()
    return P.cpu(), M.cpu(), V.cpu()


def _compare(ck, tag, p_old, lr, got, r64, r32, sl=slice(None), plain=False):
    """exp_avg, exp_avg_sq and the step (plain: p_new itself) of the elements ``sl``."""
    (gp, gm, gv), (p64, m64, v64), (p32, m32, v32) = got, r64, r32
    ck.cmp(f"{tag} exp_avg", gm[sl], m64[sl], m32[sl])
    ck.cmp(f"{tag} exp_avg_sq", gv[sl], v64[sl], v32[sl])
    if plain:
        ck.cmp(f"{tag} p_new", gp[sl], p64[sl], p32[sl])
    else:
        po = p_old.double()[sl]
        ck.cmp(f"{tag} step (p_new - p_old) / lr", (gp.double()[sl] - po) / lr, (p64[sl] - po) / lr, (p32.double()[sl] - po) / lr)


# ================================================================================================ 1. hypad_adam_step
def _adam_ref(p, g, m, v, step, lr, wd, dt):
    return manual.adam_step(p.to(dt), g.to(dt), m.to(dt), v.to(dt), step, lr, B1, B2, EPS, wd)      # (wd folded in as g + wd * p)


@pytest.mark.parametrize("n", (1, 255, 256, 257, GRID_EDGE + 257))
def test_adam_step(n):
    """n around one 256-element block and one element-block past the 2 048-block grid (the grid stride); steps 1, 2, 10 and 1000 from
    given moments; weight decay 0 and 0.1."""
    g = torch.Generator().manual_seed(n)
    cks = []
    for step in STEPS:
        for wd in WDS:
            p, grad, m, v = _euclid_data(g, n)
            ck = Ck(f"adam_step n {n} step {step} wd {wd:g}")
            _compare(ck, "", p, LR, _gpu_adam(p, grad, m, v, step, LR, wd), _adam_ref(p, grad, m, v, step, LR, wd, F64), _adam_ref(p, grad, m, v, step, LR, wd, F32))
            cks.append(ck)
    _finish(cks, f"adam_step n {n}")


def test_adam_step_at_storage_offset_one():
    g = torch.Generator().manual_seed(5)
    p, grad, m, v = _euclid_data(g, 257)
    ck = Ck("adam_step n 257 step 10 wd 0.1, p / g / m / v at storage offset 1")
    got = _gpu_adam(p, grad, m, v, 10, LR, WDS[1], dev=lambda t: _at_offset(t.cuda(), 1))
    _compare(ck, "", p, LR, got, _adam_ref(p, grad, m, v, 10, LR, WDS[1], F64), _adam_ref(p, grad, m, v, 10, LR, WDS[1], F32))
    _finish([ck], "adam_step offset 1")


# ================================================================================================ 2. / 3. hypad_radam_step
def _radam_ref(p, g, m, v, off, dim, step, lr, wd, stabilize, dt):
    """Euclidean rule everywhere, then the ball rule alone on [off, off + dim) (its exp_avg_sq is one scalar, stored repeated)."""
    P, G, M, V = (t.to(dt) for t in (p, g, m, v))
    np_, nm, nv = manual.radam_euclid_step(P, G, M, V, step, lr, B1, B2, EPS, wd)
    if dim:
        s = slice(off, off + dim)
        bp, bm, bv = manual.radam_ball_step(P[s], G[s], M[s], V[off], step, lr, B1, B2, EPS, wd, stabilize=stabilize or None)
        np_, nm, nv = np_.clone(), nm.clone(), nv.clone()
        np_[s], nm[s], nv[s] = bp, bm, bv
    return np_, nm, nv


@pytest.mark.parametrize("n", (257, GRID_EDGE + 257))
def test_radam_step_euclidean_branch(n):
    """ball_dim = 0: the Euclidean branch of the Riemannian rule (eps after the bias correction of v, weight decay inside the rule)."""
    g = torch.Generator().manual_seed(7 * n)
    cks = []
    for step in STEPS:
        for wd in WDS:
            p, grad, m, v = _euclid_data(g, n)
            ck = Ck(f"radam_step euclidean n {n} step {step} wd {wd:g}")
            _compare(ck, "", p, LR, _gpu_radam(p, grad, m, v, 0, 0, step, LR, wd, 10),
                     _radam_ref(p, grad, m, v, 0, 0, step, LR, wd, 10, F64), _radam_ref(p, grad, m, v, 0, 0, step, LR, wd, 10, F32))
            cks.append(ck)
    _finish(cks, f"radam_step euclidean n {n}")


def _ball_data(g, off, dim, radius):
    """A tensor of off + dim + 5 elements: Euclidean ones as in _euclid_data around a ball point of norm ``radius`` with a tangent first
    moment, one second moment for the whole ball and a gradient ~ N(0, 1)."""
    n = off + dim + 5
    p, grad, m, v = _euclid_data(g, n)
    s = slice(off, off + dim)
    u = torch.randn(dim, generator=g, dtype=F64)
    p[s] = (u / u.norm() * radius).float()
    grad[s] = torch.randn(dim, generator=g)
    m[s] = 0.01 * torch.randn(dim, generator=g)
    v[s] = 0.01 + 0.01 * float(torch.rand(1, generator=g))
    return p, grad, m, v


def _ball_case(tag, p, grad, m, v, off, dim, step, lr, wd, stabilize, plain=False):
    ck = Ck(f"radam_step ball dim {dim} off {off} {tag}")
    got = _gpu_radam(p, grad, m, v, off, dim, step, lr, wd, stabilize)
    r64, r32 = (_radam_ref(p, grad, m, v, off, dim, step, lr, wd, stabilize, dt) for dt in (F64, F32))
    n = p.numel()
    eu = np.r_[0:off, off + dim:n]
    _compare(ck, "euclidean elements", p, lr, got, r64, r32, eu, plain)
    _compare(ck, "ball segment", p, lr, got, r64, r32, slice(off, off + dim), plain)
    seg = got[2][off:off + dim]
    if not bool((seg == seg[0]).all()):
        j = int(torch.nonzero(seg != seg[0])[0])
        ck.failures.append(f"{ck.case}: exp_avg_sq of the ball segment is not one value repeated: element {j} is {float(seg[j]):.9g}, element 0 "
                           f"{float(seg[0]):.9g}")
    return ck, r64


@pytest.mark.parametrize("dim", (1, 2, 63, 64, 65, 128, 129, 255, 256))
def test_radam_step_ball_branch(dim):
    """Every element-per-lane class of the wave that holds the ball (64 / 128 / 256 and their neighbours), the ball at element 0, 1 and
    3 of a tensor with Euclidean elements on both sides, start radii 0, 0.5 and 0.95, stabilize 0 / 1 / 10 at step 10, weight decay 0
    and 0.1; then one step that crosses the rim."""
    g = torch.Generator().manual_seed(1000 + dim)
    cks = []
    for off in (0, 1, 3):
        for radius in (0.0, 0.5, 0.95):
            for stabilize in (0, 1, 10):
                for wd in WDS:
                    p, grad, m, v = _ball_data(g, off, dim, radius)
                    cks.append(_ball_case(f"radius {radius} stabilize {stabilize} wd {wd:g} step 10", p, grad, m, v, off, dim, 10, LR, wd, stabilize)[0])
    # the rim: |p| = 0.99, gradient and first moment pointing outward (the step is -m-hat / sqrt(v-hat)), lr = 0.5 -- the unprojected step
    # ends far outside the ball, project brings it back to its limit 1 - 4e-3.  Step 3 with stabilize 10: the second projection does
    # not run, the first alone must hold
    for off in (0, 3):
        p, grad, m, v = _ball_data(g, off, dim, 0.99)
        s = slice(off, off + dim)
        unit = p[s] / p[s].norm()
        grad[s], m[s], v[s] = -unit, -0.01 * unit, 1e-6
        ck, r64 = _ball_case("rim crossing, lr 0.5 step 3", p, grad, m, v, off, dim, 3, 0.5, 0.0, 10)
        assert abs(float(r64[0][s].norm()) - manual.MAXNORM_F32) < 1e-12, "the reference step does not end on project's limit"
        cks.append(ck)
    _finish(cks, f"radam_step ball dim {dim}")


def test_radam_step_at_the_shipped_hyper_parameters():
    """lr 5e-4, weight decay 1e-5, stabilize 10, a ball of 100 at element 3 and radius 0.93, steps 9 and 10: the plain rule on p_new."""
    g = torch.Generator().manual_seed(100)
    cks = []
    for step in (9, 10):
        p, grad, m, v = _ball_data(g, 3, 100, 0.93)
        cks.append(_ball_case(f"shipped hyper-parameters step {step}", p, grad, m, v, 3, 100, step, f32(5e-4), f32(1e-5), 10, plain=True)[0])
    _finish(cks, "radam_step shipped")


# ================================================================================================ 4. argument checks
def test_optimizer_steps_refuse_bad_arguments_and_launch_nothing():
    c = _C()
    n = 300
    bufs = [torch.full((n,), SENTINEL, device="cuda") for _ in range(4)]
    P, G, M, V = (c.ptr(t) for t in bufs)
    s = c.stream()
    hp = (LR, B1, B2, EPS, WDS[1])
    assert c.lib.hypad_radam_step(P, G, M, V, n, 0, 257, 1, *hp, 10, s) == HYPAD_EINVAL            # a ball wider than 64 lanes x 4
    assert c.lib.hypad_radam_step(P, G, M, V, n, 45, 256, 1, *hp, 10, s) == HYPAD_EINVAL           # ball_off + ball_dim > n
    assert c.lib.hypad_radam_step(P, G, M, V, n, -1, 4, 1, *hp, 10, s) == HYPAD_EINVAL
    assert c.lib.hypad_radam_step(P, G, M, V, n, 0, 0, 0, *hp, 10, s) == HYPAD_EINVAL              # step < 1
    assert c.lib.hypad_adam_step(P, G, M, V, n, 0, *hp, s) == HYPAD_EINVAL
    for k in range(4):
        a = [P, G, M, V]
        a[k] = None
        assert c.lib.hypad_adam_step(*a, n, 1, *hp, s) == HYPAD_EINVAL
        assert c.lib.hypad_radam_step(*a, n, 0, 4, 1, *hp, 10, s) == HYPAD_EINVAL
    assert c.lib.hypad_adam_step(P, G, M, V, 0, 1, *hp, s) == HYPAD_OK                             # n == 0
    assert c.lib.hypad_radam_step(P, G, M, V, 0, 0, 0, 1, *hp, 10, s) == HYPAD_OK
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in bufs)                                          # nothing ran
