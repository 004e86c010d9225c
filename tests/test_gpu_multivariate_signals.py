"""Grouped scoring of multivariate signals (hypad_row_diff_norms, hypad_zscore_clip_signals, utils.anomaly_detection_utils.
multivariate_scores_signals, main.run_signals on window-matrix datasets) against the per-signal path it replaces -- equal bit patterns,
NaNs equal where both sides have them -- and against the oracle's composition on the fixture score.npz."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import artefacts, equal, load, metrics_repr, same_bits, signal_models

pytestmark = pytest.mark.gpu

COMBINATIONS = ["sum", "mult", "uncertainty", "critic", "critic_uncertainty", "sum_uncertainty", "rec", "rec_uncertainty"]
_same_bits = functools.partial(same_bits, dtype=torch.float64)       # (every score compared here is fp64)
MV = dict(window_size_portion=0.2, window_step_size_portion=0.1, anomaly_padding=200)      # multivariate_anomaly_detection's settings


# ---------------------------------------------------------------------------------------------- hypad_row_diff_norms
@pytest.mark.parametrize("dim", [1, 51, 64, 65, 123, 150])
@pytest.mark.parametrize("rows", [1, 5, 257])
def test_row_diff_norms_equals_row_norms_of_the_fp32_difference(rows, dim):
    from hypad_amd.utils import anomaly_detection_utils as adu
    g = np.random.default_rng(rows * 1000 + dim)
    a = g.uniform(-1, 1, (rows, dim)).astype(np.float32)
    b = (a + 0.3 * g.standard_normal((rows, dim))).astype(np.float32)
    b[rows // 2] = a[rows // 2]                                     # one row with a == b
    got = adu.row_diff_norms(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
    diff = a - b
    assert diff.dtype == np.float32
    want = adu.row_norms(torch.from_numpy(diff).cuda())
    _same_bits(got, want, (rows, dim))
    assert float(got[rows // 2]) == 0.0 and (rows == 1 or float(got.max()) > 0.0)
    np.testing.assert_allclose(got.cpu().numpy(), np.linalg.norm(diff.astype(np.float64), axis=1), rtol=1e-5)


# ---------------------------------------------------------------------------------------------- hypad_zscore_clip_signals
LENGTHS = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 300_000]     # the slice-count boundaries of stat_blocks, its cap of 256 slices


def _segments(lengths, seed):
    g = np.random.default_rng(seed)
    return [3.0 + 2.0 * g.standard_normal(n) + 0.5 * np.sin(np.arange(n) / 37.0) for n in lengths]


def _offsets(lengths):
    return [0] + [int(v) for v in np.cumsum(lengths)]


def _alone(adu, seg):
    return adu.zscore_clip(torch.from_numpy(np.ascontiguousarray(seg)).cuda())


def test_zscore_clip_signals_equals_zscore_clip_per_segment():
    from hypad_amd.utils import anomaly_detection_utils as adu
    segs = _segments(LENGTHS, 1)
    off = _offsets(LENGTHS)
    x = torch.from_numpy(np.concatenate(segs)).cuda()
    got = adu.zscore_clip_signals(x, off)
    for k, seg in enumerate(segs):
        _same_bits(got[off[k]: off[k + 1]], _alone(adu, seg), ("segment", k, len(seg)))
    assert bool(torch.isnan(got[0]))                                   # one value: standard deviation 0, 0 / 0
    assert bool(torch.isfinite(got[off[2]:]).all()) and float(got[off[2]:].min()) == 1.0
    # a segment's output does not depend on the group it is scored in: alone, and in another group at another place
    for k in (3, 6, 9):
        _same_bits(adu.zscore_clip_signals(torch.from_numpy(segs[k]).cuda(), [0, len(segs[k])]), got[off[k]: off[k + 1]], ("alone", k))
    order = [9, 0, 6, 3]
    again = adu.zscore_clip_signals(torch.from_numpy(np.concatenate([segs[k] for k in order])).cuda(), _offsets([LENGTHS[k] for k in order]))
    o2 = _offsets([LENGTHS[k] for k in order])
    for j, k in enumerate(order):
        _same_bits(again[o2[j]: o2[j + 1]], got[off[k]: off[k + 1]], ("regrouped", k))


def test_zscore_clip_signals_seventy_segments_constant_and_nan():
    from hypad_amd import _C
    from hypad_amd.utils import anomaly_detection_utils as adu
    g = np.random.default_rng(2)
    lengths = [int(v) for v in g.integers(2, 40, size=70)]             # crosses the 64-segment launch boundary
    lengths[5], lengths[66] = 1500, 1100
    segs = _segments(lengths, 3)
    segs[10][:] = 0.5                                                  # constant (sums exactly): standard deviation 0, 0 / 0
    segs[65][:] = -2.0
    segs[5][700] = np.nan                                              # a NaN: its segment all NaN, no other one touched
    segs[68][1] = np.nan
    off = _offsets(lengths)
    x = torch.from_numpy(np.concatenate(segs)).cuda()
    got = adu.zscore_clip_signals(x, off)
    for k, seg in enumerate(segs):
        _same_bits(got[off[k]: off[k + 1]], _alone(adu, seg), ("segment", k, len(seg)))
    for k in (5, 68, 10, 65):
        assert bool(torch.isnan(got[off[k]: off[k + 1]]).all()), k
    rest = [k for k in range(70) if k not in (5, 10, 65, 68)]
    assert all(bool(torch.isfinite(got[off[k]: off[k + 1]]).all()) for k in rest)
    # in place equals out of place
    y = x.clone()
    nbytes = _C.lib.hypad_zscore_clip_signals_workspace_bytes(70)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _C.check(_C.lib.hypad_zscore_clip_signals(_C.ptr(y), _C.ptr(y), 70, _C.int64s(off), ws.data_ptr(), nbytes, _C.stream()), "zscore_clip_signals")
    _same_bits(y, got, "in place")


# ---------------------------------------------------------------------------------------------- multivariate_scores_signals
COUNTS = [1, 99, 100, 257, 1_300]          # 1 and 99 windows: smoothing window trunc(n * 0.01) = 0 -> NaN critic scores; 1 300: window 13
_FORWARD = {}


def _forward(S, hyp):
    """One grouped forward of small random models per (S, hyp), shared by the eight combinations and left unchanged."""
    if (S, hyp) not in _FORWARD:
        from hypad_amd.anomaly_detection import score_signals
        g = np.random.default_rng(S + int(hyp))
        models = [signal_models(k, S, 20, hyp) for k in range(len(COUNTS))]
        xs = []
        for k, n in enumerate(COUNTS):
            t = np.arange(n)[:, None] * 0.07 + np.arange(S)[None, :] * (0.11 + 0.02 * k)
            xs.append(np.clip(np.sin(t) + 0.2 * g.standard_normal((n, S)), -1, 1))           # fp64 windows, as MultivariateDataset.X holds them
        res = score_signals(xs, models, S, 20, hyp)
        torch.cuda.synchronize()
        assert tuple(res["x"].shape) == (sum(COUNTS), S) and res["x"].dtype == torch.float32
        assert torch.equal(res["x"].cpu(), torch.from_numpy(np.concatenate(xs).astype(np.float32)))
        host = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in res.items()}
        _FORWARD[(S, hyp)] = (res, host, xs)
    return _FORWARD[(S, hyp)]


@pytest.mark.parametrize("S", [150, 51])
@pytest.mark.parametrize("hyp", [True, False])
def test_multivariate_scores_signals_equals_per_signal(S, hyp, monkeypatch):
    from hypad_amd.utils import anomaly_detection_utils as adu
    res, host, xs = _forward(S, hyp)
    # (final_scores is what is compared: the host interval search that follows it in multivariate_anomaly_detection is left out)
    monkeypatch.setattr(adu, "find_anomalies", lambda *a, **k: [])
    P = SimpleNamespace(hyperbolic=hyp, signal_shape=S)
    ro = res["row_off"]
    for comb in COMBINATIONS:
        out = adu.multivariate_scores_signals(res, res["x"], comb)
        assert out["row_off"] == ro and (out["critic_scores"] is None) == (comb in ("rec", "rec_uncertainty"))
        final = out["final_scores"].cpu().numpy()
        for k, n in enumerate(COUNTS):
            a, b = ro[k], ro[k + 1]
            true = host["hyper_real"][a:b] if hyp else xs[k]             # what test_tadgan hands to the detector
            want = adu.multivariate_anomaly_detection(host["recons"][a:b], true, P, comb, list(host["critic"][a:b]))["final_scores"]
            _same_bits(final[a:b], want, (comb, k, n))
            if n < 100 and comb not in ("rec", "rec_uncertainty"):
                assert np.isnan(final[a:b]).all(), (comb, n)
            elif n > 1:
                assert np.isfinite(final[a:b]).all(), (comb, n)


# ---------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("hyp", [True, False])
def test_grouped_scores_and_intervals_meet_the_oracle(hyp):
    """score.npz cut into three segments; per segment the oracle's composition as test_multivariate_anomaly_detection composes it
    (same tolerance).  The cut 101 / 100 / 99 windows is one at which the ORACLE's scores hold an interval in both modes (worked out
    on the host from oracle.scoring and utils.intervals alone); its last segment takes the NaN critic path, and in hyperbolic mode
    the segment with the scaled rows is all NaN on both sides (the fixture's rows lie outside the unit ball).  Intervals: the bounds find_anomalies_signals extracts from the grouped scores equal those of the
    host find_anomalies on the ORACLE's scores; the interval scores follow the device-interval contract (rtol 1e-9 against the host
    find_anomalies on the same device scores -- against scores that themselves differ by 3e-4 no such bound can hold)."""
    from hypad_amd.utils import anomaly_detection_utils as adu
    from hypad_amd.utils import intervals as iv
    from hypad_amd.utils.dataloader import _yahoo_timestamps
    from oracle import scoring as osc
    fx = load("score.npz")
    S = 100
    rec_in = fx["ball_recons"].copy()
    rec_in[120:135] *= 0.2
    ro = [0, 101, 201, 300]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = {"recons": dev(rec_in), "hyper_real": dev(fx["ball_real"]) if hyp else None, "critic": dev(fx["critic"]), "row_off": ro}
    out = adu.multivariate_scores_signals(res, dev(fx["ball_real"]), "mult")
    final = out["final_scores"].cpu().numpy()
    index = [_yahoo_timestamps(ro[k + 1] - ro[k]) for k in range(3)]
    found = adu.find_anomalies_signals(out["final_scores"], ro, index_list=index, **MV)
    n_found = 0
    for k in range(3):
        a, b = ro[k], ro[k + 1]
        ra, rb = rec_in[a:b].astype(np.float64), fx["ball_real"][a:b].astype(np.float64)
        if hyp:
            with np.errstate(invalid="ignore"):
                rec = np.arccosh(1 + 2 * ((rb - ra) ** 2).sum(1) / ((1 - (rb ** 2).sum(1)) * (1 - (ra ** 2).sum(1))) + 1e-7)
        else:
            rec = np.linalg.norm(rb - ra, axis=1)
        crit = osc.final_critic_scores(fx["critic"][a:b], b - a, S)[: b - a]
        ref = np.asarray(osc.combine_scores("mult", crit, osc.zscore_clip(rec), rec_in[a:b]), dtype=np.float64).reshape(-1)
        np.testing.assert_allclose(final[a:b], ref, rtol=3e-4, atol=3e-5, err_msg=str(k))
        ref_iv = np.asarray(iv.find_anomalies(ref, index[k], fixed_threshold=True, **MV), dtype=np.float64).reshape(-1, 3)
        own_iv = np.asarray(iv.find_anomalies(final[a:b], index[k], fixed_threshold=True, **MV), dtype=np.float64).reshape(-1, 3)
        assert found[k].shape == ref_iv.shape and np.array_equal(found[k][:, :2], ref_iv[:, :2]), (k, found[k], ref_iv)
        assert np.array_equal(found[k][:, :2], own_iv[:, :2]), (k, found[k], own_iv)
        np.testing.assert_allclose(found[k][:, 2], own_iv[:, 2], rtol=1e-9, atol=0, err_msg=str(k))
        n_found += len(ref_iv)
    assert n_found >= 1


# ---------------------------------------------------------------------------------------------- run_signals
NAMES = [("fall", 600), ("walk", 450), ("sit", 130)]            # 130 windows: the shortest with a non-NaN critic chain (trunc(1.3) = 1)


def _casas_tree(d):
    rng = np.random.default_rng(3)
    base = os.path.join(d, "DATASETS", "CASAS")

    def sequences(n, phase):
        t = np.arange(n * 30) + phase
        chans = np.stack([np.sin(2 * np.pi * t / (40 + 9 * c)) + 0.05 * rng.standard_normal(t.size) for c in range(5)])       # (5, T)
        return chans.reshape(5, n, 30).transpose(1, 0, 2).astype(np.float32)                                           # (n, 5, 30)
    os.makedirs(base)
    torch.save(torch.from_numpy(sequences(600, 0)), os.path.join(base, "normal_sequences.pt"))
    for k, (name, n) in enumerate(NAMES):
        os.makedirs(os.path.join(base, "POINTS", name))
        seq = sequences(n, 1000 * (k + 1))
        lo = n // 2
        seq[lo: lo + 30] += 1.5
        gt = np.zeros((-(-n // 100), 100, 1), np.float32)
        gt.reshape(-1)[lo: lo + 30] = 1                                # the labelled stretch
        torch.save(torch.from_numpy(seq), os.path.join(base, "POINTS", name, f"{name}_sequences_id1.pt"))
        torch.save(torch.from_numpy(gt), os.path.join(base, "POINTS", name, f"{name}_groundtruth_id1.pt"))


def _cfg(hyperbolic):
    return dict(dataset="CASAS", signal="fall", epochs=1, hyperbolic=hyperbolic, signal_shape=150, lr=5e-4, batch_size=256, save_result=False,
                filename="", rec_error="dtw", combination="mult", resume=False, resume_epoch=0, load=False, new_features=False, id=1, split=1)


@pytest.mark.parametrize("hyperbolic", [True, False])
def test_run_signals_grouped_multivariate_equals_per_signal(tmp_path, monkeypatch, hyperbolic):
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    d = str(tmp_path / "data")
    _casas_tree(d)
    outs, detect_calls = {}, {}
    real_tail, real_detect = adu.multivariate_intervals, hmain._detect

    def tail(*a, **kw):                                              # both paths end in the shared tail: its result is _detect's dict
        out = real_tail(*a, **kw)
        outs.setdefault(key, []).append(out)
        return out

    def detect(*a, **kw):
        detect_calls[key] = detect_calls.get(key, 0) + 1
        return real_detect(*a, **kw)
    monkeypatch.setattr(adu, "multivariate_intervals", tail)
    monkeypatch.setattr(hmain, "_detect", detect)
    runs = {}
    for key, kw in (("grouped", {}), ("per_signal", dict(grouped_scoring=False)), ("device", dict(device_intervals=True))):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        torch.manual_seed(9)
        runs[key] = hmain.run_signals(SimpleNamespace(**_cfg(hyperbolic)), [n for n, _ in NAMES], None, d, log=lambda s_: None, **kw)
    assert detect_calls == {"per_signal": len(NAMES)}                 # grouped scoring never takes the per-signal loop
    assert all(len(outs[k]) == len(NAMES) for k in ("grouped", "per_signal", "device"))
    for (name, n), g, p, v in zip(NAMES, outs["grouped"], outs["per_signal"], outs["device"]):
        assert g["final_scores"].shape == (n,) and np.isfinite(g["final_scores"]).all(), name
        _same_bits(np.asarray(g["final_scores"]), np.asarray(p["final_scores"]), name)
        _same_bits(np.asarray(v["final_scores"]), np.asarray(p["final_scores"]), name)
        assert equal(g["intervals"], p["intervals"]), name
        assert len(p["known_anomalies"]) == 1 and g["known_anomalies"].equals(p["known_anomalies"]) and v["known_anomalies"].equals(p["known_anomalies"])
        assert metrics_repr(g["metrics"]) == metrics_repr(p["metrics"]), name
        # the device's intervals: equal bounds, scores within the device-interval contract
        assert v["intervals"].shape == p["intervals"].shape and np.array_equal(v["intervals"][:, :2], p["intervals"][:, :2]), name
        np.testing.assert_allclose(v["intervals"][:, 2], p["intervals"][:, 2], rtol=1e-9, atol=0, err_msg=name)
        for key in ("grouped", "device"):
            r, q = runs[key][name], runs["per_signal"][name]
            assert r["n_intervals"] == q["n_intervals"] and r["confusion"] == q["confusion"] and metrics_repr(r["metrics"]) == metrics_repr(q["metrics"])
    fa, fb = artefacts(tmp_path / "grouped" / "trained_models"), artefacts(tmp_path / "per_signal" / "trained_models")
    assert sorted(fa) == sorted(fb), (sorted(fa), sorted(fb))
    for f in ("recons_signal.pt", "gt_signal.pt", "critic_score.pt") + (("eucl_recons.pt", "real_hyper.pt") if hyperbolic else ()):
        assert sum(k.endswith(f) for k in fa) == len(NAMES), (f, sorted(fa))
    for k in fa:
        assert equal(fa[k], fb[k]), k


def test_cli_signals_device_intervals_on_a_multivariate_dataset(tmp_path, monkeypatch):
    import yaml
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    d = str(tmp_path / "data")
    _casas_tree(d)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(_cfg(True), f)
    called = {"fa": 0, "detect": 0, "mv": 0}
    real_fa, real_mv, real_detect = adu.find_anomalies_signals, adu.multivariate_scores_signals, hmain._detect
    monkeypatch.setattr(adu, "find_anomalies_signals", lambda *a, **k: called.__setitem__("fa", called["fa"] + 1) or real_fa(*a, **k))
    monkeypatch.setattr(adu, "multivariate_scores_signals", lambda *a, **k: called.__setitem__("mv", called["mv"] + 1) or real_mv(*a, **k))
    monkeypatch.setattr(hmain, "_detect", lambda *a, **k: called.__setitem__("detect", called["detect"] + 1) or real_detect(*a, **k))
    monkeypatch.chdir(tmp_path)
    torch.manual_seed(9)
    out = hmain.main(["--config", str(tmp_path / "cfg.yaml"), "--data-dir", d, "--signals", ",".join(n for n, _ in NAMES), "--device-intervals"])
    assert called == {"fa": 1, "detect": 0, "mv": 1}
    assert sorted(out) == sorted(n for n, _ in NAMES) and all(r["n_intervals"] >= 0 for r in out.values())
