"""The training epoch teacher-forced against fp64 oracle/manual.py under the rule of tests/sweep_common.py (errgpu <= C * err32 + F),
shared by tests/test_gpu_shape_sweep.py and tests/test_gpu_epoch_forms.py (not a conftest: the GPU files import it).

An epoch of NB minibatches and NC critic passes runs on its full optimizer state with injected noise planes.  The first and last
critic iteration and the first and last generator launch are each checked as ONE optimizer step from the state the engine had in
front of it -- taken from a shorter epoch whose losses must be the long epoch's first rows bit for bit -- against the same step of
manual.py in fp64 (and fp32, for the allowance): losses, every gradient (through Adam's first moment at step 1), both moments and
every updated parameter."""
import numpy as np
import torch

import sweep_common as sc
from oracle import manual

F64 = torch.float64
NB, NC = 3, 2
WORST = {}                     # case label -> worst errgpu / allowance of its last epoch_against_oracle call
# The kernels' second-moment weight: (1.f - beta2) in float32 = 9.99987e-4, 1.29e-5 (relative) below the 1 - 0.999 of torch.optim.Adam
# and oracle/manual.py.  See check_step's ``sq_kernel_weight``.
W2_KERNEL = 1.0 - float(np.float32(sc.BETA2))


def cu(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def engine(S, L, B, hyper, sds, seed=0, first_signal=0, flags=0):
    """An Engine holding the prefixed state dicts ``sds`` (one per signal); ``flags``: its hypad_epoch_io.flags (epoch_flags)."""
    from hypad_amd.engine import Engine
    eng = Engine(S, L, B, hyper, n_signals=len(sds), lr=sc.LR, seed=seed, first_signal=first_signal)
    eng.epoch_flags = int(flags)
    for s, sd in enumerate(sds):
        for net in sc.NETS:
            eng.load_state_dict(net, sc.net_state(sd, net), s)
    return eng


def read(eng, which, net, sig=0):
    """{prefixed name: cpu float32 tensor} of eng.params / exp_avg / exp_avg_sq."""
    src = getattr(eng, which)[net]
    out = {}
    for nm, off, shape in eng.catalogue(net):
        n = int(np.prod(shape))
        out[f"{net}.{nm}"] = src[sig, off:off + n].view(shape).cpu().clone()
    return out


def state(eng, nets, sig=0):
    """(params, exp_avg, exp_avg_sq) of ``nets`` as prefixed dicts."""
    p, m, v = {}, {}, {}
    for net in nets:
        p.update(read(eng, "params", net, sig))
        m.update(read(eng, "exp_avg", net, sig))
        v.update(read(eng, "exp_avg_sq", net, sig))
    return p, m, v


def complete(grads, params):
    """Gradients for every catalogue tensor: those manual.py does not evaluate (W_hh, never reached with T = 1) are zero."""
    return {k: grads[k] if k in grads else torch.zeros_like(params[k]) for k in params}


def check_step(ck, net, before64, before32, g64, g32, t, hyper, after, mom64=None, mom32=None, sq_kernel_weight=False):
    """One optimizer step of ``net`` from ``before`` (with moments ``mom`` or zeros) against the GPU state ``after``.
    sq_kernel_weight: compare exp_avg_sq (and nothing else) with fp64 / fp32 references that weight g^2 by W2_KERNEL, the weight the
    kernels use, instead of 1 - beta2 -- under the same rule.  For tensors whose second moment reaches ~1, where that 1.29e-5 offset
    alone exceeds the rule (critic_z at batch 256); everything else of the step stays compared with the reference's own weight."""
    P, M, V = after
    keys = [k for k in P if k.startswith(net + ".")]
    g64 = complete({k: g64[k] for k in g64 if k in keys}, {k: before64[k] for k in keys})
    g32 = complete({k: g32[k] for k in g32 if k in keys}, {k: before32[k] for k in keys})
    s64 = sc.optimizer_step(before64, g64, net, t, hyper, mom64)
    s32 = sc.optimizer_step(before32, g32, net, t, hyper, mom32)
    b1t, b2t = 1 - sc.BETA1 ** t, 1 - sc.BETA2 ** t
    for k in keys:
        p64, m64, v64, ge64 = s64[k]
        p32, m32, v32, ge32 = s32[k]
        ball = k.endswith("hyperbolic_linear.bias") and hyper
        if t == 1 and not ball:         # the gradient itself, through Adam's first moment (wd * p included for RiemannianAdam)
            ck.cmp(k + " grad", M[k] / (1 - sc.BETA1), ge64, ge32)
        else:
            ck.cmp(k + " exp_avg", M[k], m64, m32)
        if sq_kernel_weight and not ball:
            prev64 = mom64[1][k] if mom64 else torch.zeros_like(ge64)
            prev32 = mom32[1][k] if mom32 else torch.zeros_like(ge32)
            v64 = sc.BETA2 * prev64 + W2_KERNEL * ge64 * ge64
            v32 = sc.BETA2 * prev32 + W2_KERNEL * ge32 * ge32
            ck.cmp(k + " exp_avg_sq (kernel weight)", V[k], v64, v32)
        else:
            ck.cmp(k + " exp_avg_sq", V[k], v64, v32)
        if ball:
            ck.cmp(k, P[k], p64, p32)
            continue
        ok = sc.resolvable(m64, m32)
        ck.cmp(k, P[k], p64, p32, mask=ok)
        reach = 1.0 if t == 1 else np.maximum(1.0, np.abs(sc._f64(m64)) / b1t / (np.sqrt(sc._f64(v64) / b2t) + sc.ADAM_EPS))
        moved = sc._f64(P[k]) - sc._f64(before64[k])
        lim = sc.LR * (1 + 1e-3) * reach
        ck.bound(k + " (unresolved)", np.where(ok, 0.0, moved), lim)


def epoch_setup(S, L, B, k, seed, hyper=True):
    """Starting weights of k models, their window matrices, the epoch's noise planes and its shuffles (NC critic passes + 1)."""
    nit = NB * NC
    N = NB * B + 7
    w0 = [sc.init_state(S, L, hyper, seed=seed + s) for s in range(k)]
    rng = np.random.default_rng(seed)
    xw = rng.uniform(-1, 1, (k, N, S)).astype(np.float32)
    f32 = lambda a: np.asarray(a, np.float32)
    planes = dict(z_cx=f32(rng.standard_normal((nit, k, B, L))), alpha_cx=f32(rng.uniform(size=(nit, k, B, S))),
                  z_cz=f32(rng.standard_normal((nit, k, B, L))), alpha_cz=f32(rng.uniform(size=(nit, k, B, L))),
                  z_gen=f32(rng.standard_normal((NB, k, B, L))))
    perm = np.stack([rng.permutation(N)[: NB * B] for _ in range(NC + 1)]).astype(np.int32)
    return w0, xw, planes, perm


def label_of(S, L, B, k, hyper=True, flags=0):
    return f"epoch {'h' if hyper else 'e'}({S},{L},{B}) x{k}" + (f" flags {flags}" if flags else "")


def epoch_against_oracle(S, L, B, k, slots, seed=0, hyper=True, flags=0, sq_kernel_weight_nets=()):
    """The captured epoch (train_epoch_graph) of k models in the form ``flags`` (hypad_epoch_io.flags), checked for the signals
    ``slots``; the networks in ``sq_kernel_weight_nets`` have their exp_avg_sq compared as check_step's ``sq_kernel_weight``.  Returns (engine, losses, (w0, xw, planes, perm)); WORST[label] holds the worst errgpu / allowance it saw."""
    w0, xw, planes, perm = epoch_setup(S, L, B, k, seed, hyper)
    nit = NB * NC
    x, ri = cu(xw), cu(perm, torch.int32)
    dpl = {n: cu(v) for n, v in planes.items()}
    eng = engine(S, L, B, hyper, w0, seed=7, flags=flags)
    full = eng.train_epoch_graph(x, ri, NB, NC, False, noise=dpl).cpu().numpy()
    torch.cuda.synchronize()
    assert eng.status() == 0 and np.isfinite(full).all() and full.shape == (k, (2 * NC + 1) * NB, 4)
    crit_rows, gen_rows = perm[:NC].reshape(nit, B), perm[NC].reshape(NB, B)
    label = label_of(S, L, B, k, hyper, flags)

    def critics_after(m):
        """State after the first m critic iterations: an epoch of one pass of m minibatches, whose losses must be the long run's first
        2 m rows bit for bit (its m generator steps do not touch the critics)."""
        if m == nit:
            return eng
        e = engine(S, L, B, hyper, w0, seed=7, flags=flags)
        rows = np.stack([crit_rows[:m].reshape(-1), np.tile(gen_rows, (m // NB + 1, 1))[:m].reshape(-1)]).astype(np.int32)
        nz = {n: v[:m].contiguous() for n, v in dpl.items() if n != "z_gen"}
        nz["z_gen"] = dpl["z_gen"][[b % NB for b in range(m)]].contiguous()
        l = e.train_epoch(x, cu(rows, torch.int32), m, 1, False, noise=nz).cpu().numpy()
        assert e.status() == 0
        assert np.array_equal(l[:, : 2 * m], full[:, : 2 * m]), ("critic prefix", m)
        return e

    final_critics = [state(eng, ("cx", "cz"), s)[0] for s in range(k)]

    def generator_after(g):
        if g == 0:
            return None
        if g == NB:
            return eng
        e = engine(S, L, B, hyper, w0, seed=7, flags=flags)
        for s in range(k):
            for net in ("cx", "cz"):
                e.load_state_dict(net, sc.net_state(final_critics[s], net), s)
        l = e.train_epoch(x, cu(gen_rows[:g].reshape(1, -1), torch.int32), g, 0, False,
                          noise={"z_gen": dpl["z_gen"][:g].contiguous()}).cpu().numpy()
        assert np.array_equal(l, full[:, 2 * nit: 2 * nit + g]), ("generator prefix", g)
        return e

    failures, worst = [], 0.0
    for m in (0, 2 * NB - 1):
        src, dst = (critics_after(m) if m else None), critics_after(m + 1)
        if src is not None:
            assert int(src.counters[0]) == m
        for s in slots:
            ck = sc.Checker(f"{label} signal {s} critic iteration {m}")
            if m == 0:
                before = {kk: v for kk, v in w0[s].items()}
                mom = None
            else:
                p, mm, vv = state(src, ("cx", "cz"), s)
                before = dict(w0[s]); before.update(p)
                mom = (mm, vv)
            after = state(dst, ("cx", "cz"), s)
            xb = torch.from_numpy(xw[s][crit_rows[m]])
            zx, axp = torch.from_numpy(planes["z_cx"][m, s]), torch.from_numpy(planes["alpha_cx"][m, s])
            zz, azp = torch.from_numpy(planes["z_cz"][m, s]), torch.from_numpy(planes["alpha_cz"][m, s])
            refs = {}
            for dt in (F64, torch.float32):
                sd = sc.cast(before, dt)
                with torch.no_grad():
                    refs[dt] = (manual.cx_iteration(sd, xb.to(dt), zx.to(dt), axp.to(dt), hyper),
                                manual.cz_iteration(sd, xb.to(dt), zz.to(dt), azp.to(dt)), sd)
            for j, net in enumerate(("cx", "cz")):
                ck.cmp(f"{net} loss", full[s, 2 * m + j, 0], refs[F64][j][0], refs[torch.float32][j][0])
                m64 = None if mom is None else tuple(sc.cast(d, F64) for d in mom)
                check_step(ck, net, refs[F64][2], refs[torch.float32][2], refs[F64][j][1], refs[torch.float32][j][1], m + 1, hyper,
                           after, m64, mom, net in sq_kernel_weight_nets)
            failures += ck.failures
            worst = max(worst, ck.worst)
    for g in (0, NB - 1):
        src, dst = generator_after(g), generator_after(g + 1)
        for s in slots:
            ck = sc.Checker(f"{label} signal {s} generator launch {g}")
            before = dict(w0[s]); before.update(final_critics[s])
            mom = None
            if src is not None:
                assert int(src.counters[2]) == g
                p, mm, vv = state(src, ("dec", "enc"), s)
                before.update(p)
                mom = (mm, vv)
            after = state(dst, ("dec", "enc"), s)
            xb = torch.from_numpy(xw[s][gen_rows[g]])
            zg = torch.from_numpy(planes["z_gen"][g, s])
            refs = {}
            for dt in (F64, torch.float32):
                sd = sc.cast(before, dt)
                with torch.no_grad():
                    refs[dt] = (manual.dec_iteration(sd, xb.to(dt), zg.to(dt), hyper), sd)
            row = full[s, 2 * nit + g]
            ck.cmp("generator loss", row[0], refs[F64][0][0], refs[torch.float32][0][0])
            ck.cmp("hyperbolic distance" if hyper else "mse", row[1], refs[F64][0][1], refs[torch.float32][0][1])
            m64 = None if mom is None else tuple(sc.cast(d, F64) for d in mom)
            for net in ("dec", "enc"):
                check_step(ck, net, refs[F64][1], refs[torch.float32][1], refs[F64][0][2], refs[torch.float32][0][2], g + 1, hyper,
                           after, m64, mom, net in sq_kernel_weight_nets)
            failures += ck.failures
            worst = max(worst, ck.worst)
    WORST[label] = worst
    assert not failures, "\n".join(failures)
    return eng, full, (w0, xw, planes, perm)
