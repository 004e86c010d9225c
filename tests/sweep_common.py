"""Shared pieces of the shape sweep (tests/test_shape_sweep_rules.py on CPU, tests/test_gpu_shape_sweep.py on the GPU): the
comparison rule against fp64 ``oracle/manual.py``, the grid of runtime shapes, and the weights and data every shape starts from.
``Checker``, ``_ball_rows`` and ``_unaligned`` also serve tests/test_gpu_dense_layers.py; ``Ck`` (the Checker plus the reduction rule of
that file's docstring) and the guard / offset helpers at the end serve it, tests/test_gpu_lstm_seq.py and
tests/test_gpu_optimizer_steps.py.

Comparison rule.  For a compared tensor T with fp64 result ``ref64``:
    err(t) = max|t - ref64| / max(1, max|ref64|)
    err32  = err of the same oracle/manual.py computation run on CPU in fp32
    errgpu = err of the GPU result
and T passes when ``errgpu <= C * err32 + F``.  A failure names the tensor, the worst (row, column) and both errors, so that a wrong
tail column or padding stride shows up as such.

C and F were fixed once, on the anchor shapes (S, L, B) = (100, 20, 64), hyperbolic and Euclidean, which run the shipped,
specialised kernels: C = 8, F = 2e-6 (the starting point, not widened).  Observed on an MI355X at the anchors, worst
errgpu / (C * err32 + F) over every compared tensor of one critic_x, critic_z and generator iteration: 0.269 hyperbolic, 0.218
Euclidean.  The runtime shapes of the grid come out between 0.17 and 0.82 (the largest at (200, 31, 256)).  The rule is the same at
every shape; no shape gets its own constants.

A recurrence over T steps (tests/test_gpu_lstm_seq.py) passes ``steps=T``: the absolute floor becomes T * F.  F is what ONE application
of the device activations (hardware exp and reciprocal) was given; a recurrence applies them T times, and err32 already carries the
growth of rounding.  steps = 1, the default, is the rule above unchanged.

Adam's first step moves a weight by about lr * sign(g) wherever |g| sits at rounding level, so updated parameters are compared under
the rule only where the fp64 gradient is resolvable (|g64| well above the gradient's own allowance); every other element is bounded
by the distance Adam can travel in that step.
"""
import re

import numpy as np
import torch

from oracle import manual

C = 8.0
F = 2e-6
LR, BETA1, BETA2, ADAM_EPS = 5e-4, 0.9, 0.999, 1e-8
GEN_WD = 1e-5                 # RiemannianAdam's weight decay on the generator (hyperbolic mode only)

SHIPPED = {(100, 20, 64), (150, 20, 256), (123, 20, 64), (51, 20, 64)}
ANCHOR = (100, 20, 64)
# (S, L, B): every epl16_dispatch class (S <= 64 / <= 112 / <= 128 / > 128) at both of its edges, widths that are not multiples of
# 4 or 16, L from 1 to 32, B from 16 to 256, shipped widths at batches that are not shipped.  (256, 32, 32) is refused by the training
# calls (HYPAD_EUNSUPPORTED: the critic launches' LDS, test_gpu_shape_sweep.py asserts it); (256, 28, 32) is the nearest accepted shape
# at the same window, i.e. in the same row-layout class.
REFUSED = (256, 32, 32)
HYPER_GRID = [(8, 20, 64), (51, 20, 32), (64, 16, 64), (65, 20, 64), (100, 20, 48), (112, 7, 64), (113, 20, 128), (128, 32, 64),
              (129, 1, 64), (150, 20, 64), (200, 31, 256), (256, 28, 32)]
EUCL_GRID = [(33, 20, 16), (100, 20, 80), (256, 20, 64)]


def grid():
    """[(S, L, B, hyperbolic, tag)]: tag 'anchor' for the two trusted shipped shapes, 'runtime' for the rest."""
    out = [ANCHOR + (True, "anchor"), ANCHOR + (False, "anchor")]
    out += [s + (True, "runtime") for s in HYPER_GRID]
    out += [s + (False, "runtime") for s in EUCL_GRID]
    return out


def grid_id(case):
    S, L, B, hyper, tag = case
    return f"{'h' if hyper else 'e'}{S}x{L}x{B}" + ("-anchor" if tag == "anchor" else "")


NETS = ("enc", "dec", "cx", "cz")


# ------------------------------------------------------------------------------------------------ the rule
def _f64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t, dtype=np.float64)


def rel_err(got, ref64):
    """(error, flat index of the worst element) of ``got`` against ``ref64``, relative to max(1, max|ref64|)."""
    got, ref = _f64(got), _f64(ref64)
    if ref.size == 0:
        return 0.0, 0
    d = np.abs(got - ref)
    d = np.where(np.isnan(d), np.inf, d)
    i = int(np.argmax(d))
    return float(d.reshape(-1)[i]) / max(1.0, float(np.abs(ref).max())), i


def _where(shape, i):
    if len(shape) == 0:
        return "()"
    if len(shape) == 1:
        return f"(col {i} of {shape[0]})"
    r, c = np.unravel_index(i, (int(np.prod(shape[:-1])), shape[-1]))
    return f"(row {r}, col {c} of {tuple(shape)})"


class Checker:
    """Collects every rule violation of one case, so that a failure lists all the tensors that broke it."""

    def __init__(self, case=""):
        self.case, self.failures, self.worst = case, [], 0.0

    def cmp(self, name, got, ref64, ref32, mask=None, steps=1):
        g, r64, r32 = _f64(got), _f64(ref64), _f64(ref32)
        assert g.shape == r64.shape == r32.shape, (name, g.shape, r64.shape, r32.shape)
        scale = max(1.0, float(np.abs(r64).max())) if r64.size else 1.0
        if mask is not None:
            g, r64, r32 = g[mask], r64[mask], r32[mask]
            shape_idx = np.flatnonzero(mask.reshape(-1))
        if r64.size == 0:
            return
        d32 = np.abs(r32 - r64)
        dg = np.abs(g - r64)
        dg = np.where(np.isnan(dg), np.inf, dg)
        e32, i = float(d32.max()) / scale, int(np.argmax(dg))
        eg = float(dg.reshape(-1)[i]) / scale
        allow = C * e32 + steps * F
        self.worst = max(self.worst, eg / allow)
        if not eg <= allow:
            j = int(shape_idx[i]) if mask is not None else i
            floor = f"{F:g}" if steps == 1 else f"{steps} * {F:g}"
            self.failures.append(f"{self.case} {name}: errgpu {eg:.3e} > {C:g} * err32 {e32:.3e} + {floor} at {_where(_f64(ref64).shape, j)}")

    def bound(self, name, moved, limit):
        """|moved| <= limit elementwise (Adam's reach where the gradient is not resolvable)."""
        m, lim = _f64(moved), _f64(limit) * np.ones_like(_f64(moved))
        bad = ~(np.abs(m) <= lim)
        if bad.any():
            j = int(np.flatnonzero(bad.reshape(-1))[0])
            self.failures.append(f"{self.case} {name}: moved {m.reshape(-1)[j]:.3e} beyond Adam's reach {lim.reshape(-1)[j]:.3e} at "
                                 f"{_where(m.shape, j)}")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def grad_allowance(g64, g32):
    """Absolute allowance of a gradient under the rule (what a GPU gradient may be off by)."""
    g64, g32 = _f64(g64), _f64(g32)
    scale = max(1.0, float(np.abs(g64).max()))
    return (C * float(np.abs(g32 - g64).max()) / scale + F) * scale


def resolvable(g64, g32):
    """Elements whose fp64 gradient is far enough from zero that the sign and size of Adam's step are decided by it."""
    g64 = _f64(g64)
    return np.abs(g64) > np.maximum(10 * grad_allowance(g64, g32), 1e-6)


# ------------------------------------------------------------------------------------------------ weights and data
def init_state(S, L, hyperbolic, seed=0):
    """Oracle-module weights as one prefixed state dict ('enc.lstm.weight_ih_l0', ...), float32, with the hyperbolic head moved off
    its tiny initialisation (weight x 50, bias x 10: the ball bias then has lambda != 2)."""
    from oracle import tadgan as ot
    torch.manual_seed(seed)
    mods = dict(enc=ot.Encoder(S, L), dec=ot.Decoder(S, L, hyperbolic), cx=ot.CriticX(S, L), cz=ot.CriticZ(L))
    sd = {}
    for k, m in mods.items():
        for n, v in m.state_dict().items():
            sd[f"{k}.{n}"] = v.detach().clone().float()
    if hyperbolic:
        sd["dec.hyperbolic_linear.weight"] = sd["dec.hyperbolic_linear.weight"] * 50
        sd["dec.hyperbolic_linear.bias"] = sd["dec.hyperbolic_linear.bias"] * 10
    return sd


def net_state(sd, net):
    p = net + "."
    return {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}


def cast(sd, dtype):
    return {k: v.to(dtype) for k, v in sd.items()}


def iteration_data(S, L, B, seed=0):
    """x (B, S) in [-1, 1], z (B, L) ~ N(0, 1), alpha_x (B, S), alpha_z (B, L) in [0, 1): float32."""
    g = torch.Generator().manual_seed(1000 * S + 10 * L + B + seed)
    x = torch.rand(B, S, generator=g, dtype=torch.float64).float() * 2 - 1
    z = torch.randn(B, L, generator=g)
    return x, z, torch.rand(B, S, generator=g), torch.rand(B, L, generator=g)


def rand_masks(gen, B, p, n, width):
    return [(torch.rand(B, width, generator=gen) >= p).float() / (1 - p) for _ in range(n)]


# ------------------------------------------------------------------------------------------------ references
def iterations(sd, x, z, ax, az, hyperbolic, masks=None, critics_after=None):
    """The three iterations of oracle/manual.py in the dtype of ``sd`` (critic_x, critic_z at sd; the generator at sd with the
    critics replaced by ``critics_after`` if given).  masks: None or dict(cx=..., cz=..., dec=...) in manual's formats."""
    masks = masks or {}
    dt = next(iter(sd.values())).dtype
    x, z, ax, az = (t.to(dt) for t in (x, z, ax, az))
    with torch.no_grad():
        lx, gx = manual.cx_iteration(sd, x, z, ax, hyperbolic, masks.get("cx"))
        lz, gz = manual.cz_iteration(sd, x, z, az, masks.get("cz"))
        sd2 = dict(sd)
        if critics_after is not None:
            sd2.update(cast(critics_after, dt))
        ld, aux, gd = manual.dec_iteration(sd2, x, z, hyperbolic, masks.get("dec"))
    return dict(cx=(lx, gx), cz=(lz, gz), dec=(ld, aux, gd), sd_dec=sd2)


def optimizer_step(sd, grads, net, t, hyperbolic, moments=None):
    """One optimizer step of network ``net`` from the state ``sd`` (+ optional (exp_avg, exp_avg_sq) dicts keyed like sd): Adam for
    the critics and the Euclidean generator, RiemannianAdam (Euclidean branch + ball branch for the head bias) for the hyperbolic
    generator.  Returns {key: (param, exp_avg, exp_avg_sq, effective gradient)}."""
    out = {}
    gen = net in ("enc", "dec")
    for k, g in grads.items():
        if not k.startswith(net + "."):
            continue
        p = sd[k]
        m, v = (moments[0][k], moments[1][k]) if moments else (torch.zeros_like(p), torch.zeros_like(p))
        if gen and hyperbolic:
            if k.endswith("hyperbolic_linear.bias"):
                vs = v.reshape(-1)[0] if moments else torch.zeros((), dtype=p.dtype)
                np_, nm, nv = manual.radam_ball_step(p, g, m, vs, t, LR, BETA1, BETA2, ADAM_EPS, wd=GEN_WD)
                out[k] = (np_, nm, nv * torch.ones_like(p), g + GEN_WD * p)
            else:
                np_, nm, nv = manual.radam_euclid_step(p, g, m, v, t, LR, BETA1, BETA2, ADAM_EPS, wd=GEN_WD)
                out[k] = (np_, nm, nv, g + GEN_WD * p)
        else:
            np_, nm, nv = manual.adam_step(p, g, m, v, t, LR, BETA1, BETA2, ADAM_EPS)
            out[k] = (np_, nm, nv, g)
    return out


# ------------------------------------------------------------------------------------------------ data of the row-kernel sweeps
def _ball_rows(g, rows, dim, tangent=False, zero_row=True, edge=True, radius=0.95):
    """Rows inside the ball at radii up to ``radius``, one on the 1 - 1e-3 norm (beyond project's limit; edge=False: none), one zero
    row; tangent=True: rows for expmap0, one with norm above 15 (the tanh clamp)."""
    a = torch.randn(rows, dim, generator=g, dtype=torch.float64)
    a = a / a.norm(dim=1, keepdim=True).clamp_min(1e-300)
    if tangent:
        r = torch.rand(rows, 1, generator=g, dtype=torch.float64) * 3
        if rows >= 3:
            r[1] = 16.0 + rows % 7
    else:
        r = torch.rand(rows, 1, generator=g, dtype=torch.float64) * radius
        if rows >= 3 and edge:
            r[1] = 1 - 1e-3
    a = a * r
    if rows >= 2 and zero_row:
        a[-1] = 0
    return a.float()


def _unaligned(t):
    """A contiguous view at storage offset 1 of a larger buffer (the kernels' al == false path)."""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------------------------ the layer sweeps' checker and buffers
SENTINEL = 12345.0
NAN = float("nan")


class Ck(Checker):
    """The Checker plus the reduction rule (tests/test_gpu_dense_layers.py's docstring); for the weights-stationary LSTM layer
    (``tiles=(rows, waves)``) a failure also names the 16-row tile of its worst row and which iteration of its wave's walk that tile
    is."""

    def __init__(self, case="", tiles=None):
        super().__init__(case)
        self.rworst = 0.0
        self.tstep = None
        if tiles:
            rows, nw = tiles
            ntiles = (rows + 15) // 16
            self.nw, self.tstep = nw, min(128, -(-ntiles // nw)) * nw      # hypad_lstm_bidir_fwd: at most 128 slices of `nw` waves per direction

    def _tile_note(self, first):
        for i in range(first, len(self.failures)):
            m = re.search(r"\(row (\d+),", self.failures[i])
            if m and self.tstep:
                tile = int(m.group(1)) // 16
                self.failures[i] += (f" [tile {tile}: iteration {tile // self.tstep} (from 0) of wave {tile % self.tstep % self.nw} in slice "
                                     f"{tile % self.tstep // self.nw}, tiles {self.tstep} apart]")

    def cmp(self, name, got, ref64, ref32, mask=None, steps=1):
        n = len(self.failures)
        super().cmp(name, got, ref64, ref32, mask, steps)
        self._tile_note(n)

    def red(self, name, got, ref64, abs_terms, rows, summand_allow=0.0):
        g, r, t = _f64(got), _f64(ref64), _f64(abs_terms)
        assert g.shape == r.shape == t.shape, (name, g.shape, r.shape, t.shape)
        if r.size == 0:
            return
        scale = max(1.0, float(np.abs(r).max()))
        allow = (summand_allow + (rows + 4) * 2.0 ** -24 * t) / scale
        d = np.abs(g - r) / scale
        d = np.where(np.isnan(d), np.inf, d)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(d == 0, 0.0, d / allow)                       # (no allowance at all -- a sum over no rows -- takes exact zeros)
        i = int(np.argmax(ratio))
        worst = float(ratio.reshape(-1)[i])
        self.rworst = max(self.rworst, worst)
        if not worst <= 1.0:
            self.failures.append(f"{self.case} {name}: error {d.reshape(-1)[i]:.3e} > reduction allowance {allow.reshape(-1)[i]:.3e} "
                                 f"over {rows} rows at {_where(r.shape, i)}")

    def report(self, sweep="dense sweep"):
        print(f"\n{sweep} {self.case}: worst errgpu / allowance {self.worst:.3f}, worst reduction error / allowance {self.rworst:.3f}")


def _leaf(t, dt):
    """A fresh leaf of dtype ``dt`` (never the tensor itself: .to() returns its argument when the dtype already matches)."""
    return t.detach().to(dt).clone().requires_grad_(True)


def _at_offset(t, off):
    """A contiguous copy of ``t`` at storage offset ``off`` floats of a larger buffer."""
    buf = torch.empty(t.numel() + off, device="cuda")
    v = buf[off:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * off) % 16
    return v


def _guarded(shape, offset):
    """A NaN-filled (shape) view at storage offset ``offset`` floats with one sentinel float in front of it and one behind."""
    n = int(np.prod(shape))
    buf = torch.full((offset + n + 1,), NAN, device="cuda")
    buf[offset - 1] = SENTINEL
    buf[offset + n] = SENTINEL
    v = buf[offset:offset + n].view(shape)
    assert v.data_ptr() % 64 == (4 * offset) % 64
    return buf, v


def _guards_intact(buf, offset):
    return float(buf[offset - 1]) == SENTINEL and float(buf[-1]) == SENTINEL
