"""Grouped scoring of many trained signals (anomaly_detection.score_signals, utils.anomaly_detection_utils.hyperbolic_scores_signals,
main.run_signals(grouped_scoring=True)) against the per-signal path it replaces: equal bit patterns (NaNs equal where both sides have
them), and the reference's numbers for the grouped forward (fixture fwd_S100_B64.npz, oracle.tadgan)."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import artefacts, csv_signals, equal, load, maxdiff, metrics_repr, oracle_models, same_bits, signal_models, sub_state

pytestmark = pytest.mark.gpu


class _Series:
    """What score_signals takes from a SignalDataset: series_windows() = (series, windows, 1)."""
    def __init__(self, series, n):
        self.series, self.n = series, n

    def series_windows(self, device="cuda"):
        return self.series, self.n, 1


def _check_group(counts, S, L, hyp, series_view, seed=0):
    from hypad_amd.anomaly_detection import score_signals, score_windows
    rng = np.random.default_rng(seed)
    models = [signal_models(k, S, L, hyp) for k in range(len(counts))]
    xs, singles = [], []
    for k, n in enumerate(counts):
        series = np.clip(np.sin(np.arange(n + S - 1) * (0.05 + 0.01 * k)) + 0.1 * rng.standard_normal(n + S - 1), -1, 1).astype(np.float32)
        win = series[np.arange(n)[:, None] + np.arange(S)[None, :]]
        if series_view:
            dev = torch.from_numpy(series).cuda()
            xs.append(_Series(dev, n))
            singles.append(score_windows(torch.empty(n, S), *models[k], S, L, hyp, series=dev))
        else:
            xs.append(win[:, :, None])
            singles.append(score_windows(torch.from_numpy(win), *models[k], S, L, hyp))
    res = score_signals(xs, models, S, L, hyp)
    torch.cuda.synchronize()
    assert res["row_off"] == list(np.cumsum([0] + list(counts)))
    for k in range(len(counts)):
        a, b = res["row_off"][k], res["row_off"][k + 1]
        for key in ("recons", "eucl", "hyper_real", "critic", "rowdist"):
            if singles[k][key] is None:
                assert res[key] is None
                continue
            same_bits(res[key][a:b], singles[k][key], (counts, k, key))


@pytest.mark.parametrize("S,L", [(100, 20), (150, 20), (48, 12)])
@pytest.mark.parametrize("hyp", [True, False])
@pytest.mark.parametrize("series_view", [True, False])
def test_grouped_forward_equals_single_model(S, L, hyp, series_view):
    # both tile forms at the reference shape (65 541 windows in the group: the 32-window form), ragged tiles everywhere
    _check_group([1, 15, 16, 17, 33, 65_541], S, L, hyp, series_view)
    _check_group([17], S, L, hyp, series_view, seed=1)
    _check_group([1, 33, 300], S, L, hyp, series_view, seed=2)


def test_grouped_forward_forty_signals():
    # more signals than one training group (32): 40 models, ragged counts
    rng = np.random.default_rng(3)
    counts = [int(v) for v in rng.integers(1, 400, size=40)]
    counts[7] = 1
    _check_group(counts, 100, 20, True, True, seed=3)
    _check_group(counts, 100, 20, False, False, seed=4)


def test_engine_arenas_score_as_the_modules():
    from hypad_amd.anomaly_detection import score_signals
    from hypad_amd.engine import Engine
    S, L = 100, 20
    models = [signal_models(k, S, L, True) for k in range(3)]
    eng = Engine(S, L, 64, True, n_signals=3)
    for k, (enc, dec, cx) in enumerate(models):
        for net, m in (("enc", enc), ("dec", dec), ("cx", cx)):
            eng.params[net][k].copy_(m.arena())
    x = [np.random.default_rng(k).uniform(-1, 1, (n, S)).astype(np.float32) for k, n in enumerate((5, 70, 19))]
    a = score_signals(x, models, S, L, True)
    b = score_signals(x, eng, S, L, True)
    for key in ("recons", "eucl", "hyper_real", "critic", "rowdist"):
        same_bits(a[key], b[key], key)


def test_grouped_forward_meets_the_reference_numbers():
    from hypad_amd.anomaly_detection import score_signals
    from hypad_amd.models import tadgan
    from oracle import gmath as og
    S, L, TOL = 100, 20, 1e-4
    fx = load("fwd_S100_B64.npz")
    g = np.random.default_rng(5)
    fxs = [fx] + [{k: (v + 0.01 * g.standard_normal(v.shape)).astype(v.dtype) if k.split(".")[0] in ("enc", "dec", "cx") else v
                   for k, v in fx.items()} for _ in range(2)]
    models = []
    for f in fxs:
        enc, dec, cx = tadgan.Encoder(S, L), tadgan.Decoder(S, L, True), tadgan.CriticX(S, L)
        enc.load_state_dict(sub_state(f, "enc")); dec.load_state_dict(sub_state(f, "dec")); cx.load_state_dict(sub_state(f, "cx"))
        models.append(tuple(m.cuda().eval() for m in (enc, dec, cx)))
    x0 = fx["x"].reshape(64, S).astype(np.float32)
    x1 = g.uniform(-1, 1, (37, S)).astype(np.float32)
    x2 = g.uniform(-1, 1, (70, S)).astype(np.float32)
    res = score_signals([x0, x1, x2], models, S, L, True)
    torch.cuda.synchronize()
    ro = res["row_off"]
    want0 = {"recons": fx["s0_hyper"].reshape(64, S), "eucl": fx["s0_eucl"].reshape(64, S), "hyper_real": fx["head_x"], "critic": fx["cx_x"].reshape(64),
             "rowdist": og.rowwise_poincare_distance(torch.from_numpy(fx["head_x"]), torch.from_numpy(fx["s0_hyper"].reshape(64, S))).numpy()}
    for k, ref in want0.items():
        assert maxdiff(res[k][ro[0]:ro[1]].cpu().numpy(), ref) < TOL, k
    for s, (f, x) in enumerate(((fxs[1], x1), (fxs[2], x2)), start=1):
        enc, dec, cx, _ = [m.eval() for m in oracle_models(f, S, True)]
        with torch.no_grad():
            xs = torch.from_numpy(x.astype(np.float64)).reshape(-1, S, 1)
            hyper, eucl = dec(enc(xs))
            hreal = dec.hyperbolic_linear(xs.reshape(-1, S).float())
            want = {"recons": hyper.reshape(-1, S), "eucl": eucl.reshape(-1, S), "hyper_real": hreal, "critic": cx(xs).reshape(-1)}
            want["rowdist"] = og.rowwise_poincare_distance(want["hyper_real"], want["recons"])
        for k, ref in want.items():
            ref = ref.numpy()
            assert maxdiff(res[k][ro[s]:ro[s + 1]].cpu().numpy(), ref) < TOL * max(1.0, float(np.abs(ref).max())), (s, k)


@pytest.mark.parametrize("combination", ["sum", "mult", "uncertainty", "critic", "critic_uncertainty", "sum_uncertainty", "rec", "rec_uncertainty"])
def test_grouped_hyperbolic_chain_equals_per_signal(combination):
    from hypad_amd.utils import anomaly_detection_utils as adu
    S = 100
    counts = [50, 1, 120, 333, 1_500]              # 50 and 1 windows: smoothing window trunc(n * 0.01) = 0 -> NaN segments
    g = torch.Generator(device="cuda").manual_seed(11)
    n = sum(counts)
    res = {"recons": (0.05 * torch.randn(n, S, device="cuda", generator=g)).contiguous(),
           "hyper_real": (0.05 * torch.randn(n, S, device="cuda", generator=g)).contiguous(),
           "critic": torch.randn(n, device="cuda", generator=g), "row_off": list(np.cumsum([0] + counts))}
    out = adu.hyperbolic_scores_signals(res, combination)
    torch.cuda.synchronize()
    ro = out["row_off"]
    for k in range(len(counts)):
        a, b = ro[k], ro[k + 1]
        rec, real, crit = res["recons"][a:b].cpu().numpy(), res["hyper_real"][a:b].cpu().numpy(), res["critic"][a:b].cpu().numpy()
        want = adu.hyperbolic_scores(rec, real, list(crit), S, combination)
        same_bits(out["final_scores"][a:b], torch.from_numpy(np.asarray(want)), (combination, k))
        if out["critic_scores"] is not None:
            fc = adu.final_critic_scores(list(crit), real)
            same_bits(out["critic_scores"][a + k * (S - 1): b + (k + 1) * (S - 1)], torch.from_numpy(fc), (combination, k, "critic"))
            if counts[k] < 100:
                assert bool(torch.isnan(out["critic_scores"][a + k * (S - 1): b + (k + 1) * (S - 1)]).all())


def _metrics(r):
    return metrics_repr(r["metrics"])


@pytest.mark.parametrize("hyperbolic", [True, False])
def test_run_signals_grouped_equals_per_signal(tmp_path, monkeypatch, hyperbolic):
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    d = tmp_path / "data"
    d.mkdir()
    names = [("sa", 700), ("sb", 520), ("sc", 180)]          # 180 - 100 windows: a smoothing window of 0 (NaN critic scores)
    csv_signals(d, names)
    cfg = dict(dataset="NAB", signal="sa", epochs=1, hyperbolic=hyperbolic, signal_shape=100, lr=5e-4, batch_size=64, save_result=False,
               filename="", rec_error="dtw", combination="mult", interval=600, unique_dataset=True, resume=False, resume_epoch=0, load=False)
    seen = {}
    real_find = adu.find_anomalies

    def spy(scores, index, *a, **kw):
        seen.setdefault(key, []).append(np.array(scores, dtype=np.float64))
        return real_find(scores, index, *a, **kw)
    monkeypatch.setattr(adu, "find_anomalies", spy)
    runs = {}
    for key, grouped in (("grouped", True), ("per_signal", False)):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        torch.manual_seed(9)
        runs[key] = hmain.run_signals(SimpleNamespace(**cfg), [n for n, _ in names], None, str(d), log=lambda s_: None, grouped_scoring=grouped)
    assert len(seen["grouped"]) == len(seen["per_signal"]) == len(names)
    for a, b in zip(seen["grouped"], seen["per_signal"]):
        assert a.tobytes() == b.tobytes()
    for name, _ in names:
        ga, pa = runs["grouped"][name], runs["per_signal"][name]
        assert ga["confusion"] == pa["confusion"] and _metrics(ga) == _metrics(pa) and ga["n_intervals"] == pa["n_intervals"]
    fa, fb = artefacts(tmp_path / "grouped" / "trained_models"), artefacts(tmp_path / "per_signal" / "trained_models")
    assert sorted(fa) == sorted(fb) and any(k.endswith("anomalies.csv") for k in fa) and any(k.endswith("recons_signal.pt") for k in fa)
    if hyperbolic:
        assert any(k.endswith("critic_scores.pickle") for k in fa)
    for k in fa:
        assert equal(fa[k], fb[k]), k


def test_cli_per_signal_scoring_flag(tmp_path, monkeypatch):
    import yaml
    from hypad_amd import main as hmain
    d = tmp_path / "data"
    d.mkdir()
    csv_signals(d, [("sa", 400), ("sb", 300)])
    cfg = dict(dataset="NAB", signal="sa", epochs=1, hyperbolic=True, signal_shape=100, lr=5e-4, batch_size=64, save_result=False, filename="",
               rec_error="dtw", combination="mult", interval=600, unique_dataset=True, resume=False, resume_epoch=0, load=False)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    called = []
    real = hmain._detect_grouped
    monkeypatch.setattr(hmain, "_detect_grouped", lambda *a, **k: called.append(1) or real(*a, **k))
    monkeypatch.chdir(tmp_path)
    out = {}
    for flag in ([], ["--per-signal-scoring"]):
        torch.manual_seed(9)
        out[bool(flag)] = hmain.main(["--config", str(tmp_path / "cfg.yaml"), "--data-dir", str(d), "--signals", "sa,sb"] + flag)
    assert called == [1]
    assert {k: (v["confusion"], _metrics(v)) for k, v in out[False].items()} == {k: (v["confusion"], _metrics(v)) for k, v in out[True].items()}
