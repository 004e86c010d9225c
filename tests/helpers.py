"""Shared helpers for the test-suite (fixtures -> oracle modules)."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def sub_state(fx, prefix, wkey=None):
    """Extract one network's state_dict from a fixture ('enc.' keys, or 'w0.enc.' with wkey='w0')."""
    pre = (wkey + "." if wkey else "") + prefix + "."
    return {k[len(pre):]: torch.from_numpy(np.array(v)) for k, v in fx.items() if k.startswith(pre)}


def oracle_models(fx, S, hyperbolic=True, wkey=None, L=20):
    from oracle import tadgan
    enc = tadgan.Encoder(S, L)
    dec = tadgan.Decoder(S, L, hyperbolic)
    cx = tadgan.CriticX(S, L)
    cz = tadgan.CriticZ(L)
    enc.load_state_dict(sub_state(fx, "enc", wkey))
    dsd = sub_state(fx, "dec", wkey)
    if not hyperbolic:
        dsd = {k: v for k, v in dsd.items() if not k.startswith("hyperbolic_linear")}
    dec.load_state_dict(dsd)
    cx.load_state_dict(sub_state(fx, "cx", wkey))
    cz.load_state_dict(sub_state(fx, "cz", wkey))
    return enc, dec, cx, cz


def params_ns(B=64, S=100, hyperbolic=True, lr=5e-4):
    return SimpleNamespace(batch_size=B, signal_shape=S, latent_space_dim=20, lr=lr, hyperbolic=hyperbolic)


def _np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def maxdiff(a, b):
    a, b = np.asarray(_np(a), dtype=np.float64), np.asarray(_np(b), dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def same_bits(a, b, what="", dtype=None):
    """a and b (tensors or arrays, fp32 or fp64) have one shape, one dtype -- ``dtype`` where given -- and equal bit patterns, NaNs included."""
    a, b = (torch.as_tensor(_np(v)).contiguous() for v in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype and dtype in (None, a.dtype), (what, a.shape, b.shape, a.dtype, b.dtype, dtype)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), (what, "NaN positions differ", int(torch.isnan(a).sum()), int(torch.isnan(b).sum()))
    ba, bb = (t.reshape(-1).view(torch.int64 if t.dtype == torch.float64 else torch.int32) for t in (a, b))
    bad = torch.nonzero(ba != bb).reshape(-1)
    assert not bad.numel(), (what, int(bad.numel()), "first at", int(bad[0]), float(a.reshape(-1)[bad[0]]), float(b.reshape(-1)[bad[0]]), maxdiff(a, b))


def signal_models(k, S, L, hyp):
    """Signal k's (encoder, decoder, critic_x) of a group of small random models, on the device."""
    from hypad_amd.models import tadgan
    torch.manual_seed(1000 + k)
    return tuple(m.cuda().eval() for m in (tadgan.Encoder(S, L), tadgan.Decoder(S, L, hyp), tadgan.CriticX(S, L)))


def csv_signals(d, lengths):
    """<name>.csv per (name, length) under ``d`` -- a sine with noise and one raised stretch -- and anomalies.csv labelling that stretch."""
    t0 = 1_400_000_000
    rows = []
    for k, (name, n) in enumerate(lengths):
        rng = np.random.default_rng(70 + k)
        tt = np.arange(n)
        v = np.sin(2 * np.pi * tt / (55.0 + 9 * k)) + 0.05 * rng.standard_normal(n)
        v[n // 2: n // 2 + 25] += 1.5
        with open(d / f"{name}.csv", "w") as f:
            f.write("timestamp,value\n" + "\n".join(f"{t0 + 600 * i},{x:.6f}" for i, x in zip(tt, v)) + "\n")
        rows.append('%s,"[[%d, %d]]"' % (name, t0 + 600 * (n // 2 - 5), t0 + 600 * (n // 2 + 30)))
    with open(d / "anomalies.csv", "w") as f:
        f.write("signal,events\n" + "\n".join(rows) + "\n")


def artefacts(root):
    """Every file the runs wrote below ./trained_models except the model weights, loaded."""
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            p = os.path.join(dirpath, f)
            key = os.path.relpath(p, root)
            if f.endswith(".pt") and f not in ("recons_signal.pt", "gt_signal.pt", "critic_score.pt", "eucl_recons.pt", "real_hyper.pt"):
                continue
            if f.endswith(".pt"):
                out[key] = torch.load(p, weights_only=False)
            elif f.endswith(".pickle"):
                with open(p, "rb") as fh:
                    out[key] = pickle.load(fh)
            else:
                with open(p) as fh:
                    out[key] = fh.read()
    return out


def equal(a, b):
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b))
    return a == b


def metrics_repr(m):
    """A metrics dict in a form where NaN equals NaN (f1 of a run without any true positive)."""
    return None if m is None else repr(sorted(m.items()))
