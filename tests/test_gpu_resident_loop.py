"""The resident epoch loop of train_tadgan_resident and train_signals_resident where tests/test_gpu_signals_r4.py does not reach: a
repair on the path that finishes every epoch before the next is queued (shuffles drawn on the host), alone and as a group of one."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
S, B = 100, 64


def windows(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n + S - 1)
    series = np.clip(np.sin(2 * np.pi * t / (40.0 + 7 * seed)) + 0.05 * rng.standard_normal(len(t)), -1, 1)
    return series[np.arange(n)[:, None] + np.arange(S)[None, :]]


def P_(epochs, **more):
    return SimpleNamespace(**{**dict(batch_size=B, signal_shape=S, latent_space_dim=20, lr=5e-4, hyperbolic=True, resume=False, resume_epoch=0,
                                     epochs=epochs, dataset="T", signal="x"), **more})


def models(seed):
    from hypad_amd.models import tadgan
    torch.manual_seed(seed)                                      # (train.py:415-426 construction order, as train_signals_resident builds them)
    return [m.cuda().train() for m in (tadgan.Encoder(S, 20), tadgan.Decoder(S, 20, True), tadgan.CriticX(S, 20), tadgan.CriticZ(20))]


def weights(mods):
    return [{k: v.detach().cpu().clone() for k, v in m.state_dict().items()} for m in mods]


def assert_same_weights(a, b):
    assert len(a) == len(b)
    for wa, wb in zip(a, b):
        assert sorted(wa) == sorted(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)


def test_a_give_up_is_repaired_where_every_epoch_is_finished_before_the_next(tmp_path, monkeypatch):
    """Engine.SHUFFLE_MAX_WINDOWS + 4 windows (64 minibatches): the smallest signal whose shuffles are drawn on the host, so that
    epoch e is finished before epoch e + 1 is queued and a repair covers exactly the epoch just finished.  A resident critic launch that
    gives up in epoch 0 (the test bits of hypad_epoch_io.flags: the library's own bounded-wait status path) is repeated launch by launch
    and counted once; histories and final weights equal those of a run in the per-iteration form from the start -- through
    train_tadgan_resident, through a one-signal train_signals_resident, and between the two.  (No checkpoint files here:
    docs/history/resident_loop.md on what a checkpoint next to a repair does on this path.)"""
    from hypad_amd import _C
    from hypad_amd import train as ht
    from hypad_amd.engine import Engine
    monkeypatch.chdir(tmp_path)
    data = windows(Engine.SHUFFLE_MAX_WINDOWS + 4, 8)
    assert len(data) // B == 64
    one, grp = [], []
    for flags in (_C.EPOCH_PER_ITERATION, 3 << _C.EPOCH_TEST_GIVE_UP_SHIFT):
        mods = models(300)
        h = ht.train_tadgan_resident(data, *mods, n_epochs=2, params=P_(2, epoch_flags=flags), seed=13, log=None)
        one.append((vars(h), weights(mods)))
        r = ht.train_signals_resident([data], P_(2, epoch_flags=flags), names=["a"], seed=13, init_seed=300, log=None, save=False)["a"]
        assert r["stream"] == 0
        grp.append((r["history"], weights(r["modules"])))
    for (ha, wa), (hb, wb) in (one, grp):
        assert ha.pop("repairs") == 0 and hb.pop("repairs") == 1
        assert ha == hb and len(hb["cx"]) == 2 and np.isfinite(hb["cx"] + hb["cz"] + hb["dec"] + hb["hyper"]).all()
        assert_same_weights(wa, wb)
    assert one[1][0] == grp[1][0]                                    # ("repairs" popped above)
    assert_same_weights(one[1][1], grp[1][1])
