"""Grouped Euclidean (TadGAN) scoring -- hypad_unroll_median_signals, hypad_rec_scores_signals, utils.anomaly_detection_utils
.euclidean_scores_signals and the Euclidean branch of main._detect_grouped -- against the single-signal functions on each signal
alone: the same bit pattern, NaN where and only where the other side has NaN; and against the reference's numbers (fixtures
score.npz / score_area_dtw.npz) at the tolerance the single-signal path is held to."""
import math
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import artefacts, csv_signals, equal, load, maxdiff, same_bits

pytestmark = pytest.mark.gpu

KINDS = ("point", "area", "dtw")
SENT32, SENT64 = -12345.5, -98765.25


def _offsets(counts):
    return [int(v) for v in np.cumsum([0] + list(counts))]


def _unroll_signals(y_hat, row_off, S):
    """hypad_unroll_median_signals into a buffer with one sentinel in front of and behind the group."""
    from hypad_amd import _C
    from hypad_amd.utils import anomaly_detection_utils as adu
    t_off = adu.timestep_offsets(row_off, S)
    buf = torch.full((t_off[-1] + 2,), SENT32, device="cuda", dtype=torch.float32)
    med = buf[1:-1]
    _C.check(_C.lib.hypad_unroll_median_signals(_C.ptr(y_hat), _C.ptr(med), len(row_off) - 1, _C.int64s(row_off), S, _C.stream()), "unroll_median_signals")
    torch.cuda.synchronize()
    assert float(buf[0]) == SENT32 and float(buf[-1]) == SENT32
    return med, t_off


def _check_unroll(counts, S, seed, decimals=False):
    from hypad_amd.utils import anomaly_detection_utils as adu
    g = torch.Generator(device="cuda").manual_seed(seed)
    y_hat = torch.randn(sum(counts), S, device="cuda", generator=g)
    if decimals:                                       # two decimals: ties on every anti-diagonal, the two-pivot shortcut has to fall back
        y_hat = (torch.round(y_hat * 100) / 100).contiguous()
    row_off = _offsets(counts)
    med, t_off = _unroll_signals(y_hat, row_off, S)
    for k in range(len(counts)):
        part = y_hat[row_off[k]: row_off[k + 1]]
        got = med[t_off[k]: t_off[k + 1]]
        same_bits(got, adu.unroll_predictions(part, with_summary=True)[0], (S, k, counts[k], "with summary"))
        same_bits(got, adu.unroll_predictions(part, with_summary=False)[0], (S, k, counts[k], "median only"))


@pytest.mark.parametrize("S", [48, 100, 150, 256])
def test_segmented_unroll_median_equals_single_signal(S):
    _check_unroll([1, 15, 16, 17, 33, 127, 128, 129, 300, 65_541], S, seed=S)
    rng = np.random.default_rng(S)
    ragged = [int(v) for v in rng.integers(1, 400, size=40)]
    ragged[7] = 1
    _check_unroll(ragged, S, seed=S + 1)
    _check_unroll([int(v) for v in rng.integers(1, 40, size=70)], S, seed=S + 2)      # two launches: 64 + 6 segments


@pytest.mark.parametrize("S", [100, 256])
def test_segmented_unroll_median_with_ties(S):
    _check_unroll([1, 33, 127, 300, 129, 2_000], S, seed=7, decimals=True)


def _series(n, S, k, rng, dtype=np.float32):
    t = np.arange(n + S - 1)
    return np.clip(np.sin(t * 2 * np.pi / (37.0 + 3 * k)) + 0.1 * rng.standard_normal(n + S - 1), -1, 1).astype(dtype)


def _rec_scores_signals(true, median, row_off, S, kinds=KINDS, score_window=10):
    """hypad_rec_scores_signals, every output with one sentinel in front of and behind the group."""
    from hypad_amd import _C
    total = true.numel()
    bufs = {k: torch.full((total + 2,), SENT64, device="cuda", dtype=torch.float64) for k in kinds}
    outs = {k: b[1:-1] for k, b in bufs.items()}
    offs = _C.int64s(row_off)
    nbytes = _C.lib.hypad_rec_scores_signals_workspace_bytes(len(row_off) - 1, offs, S)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0x5a
    _C.check(_C.lib.hypad_rec_scores_signals(sum(_C.REC_KINDS[k] for k in kinds), _C.ptr(true), _C.ptr(median), _C.ptr(outs.get("point")),
                                             _C.ptr(outs.get("area")), _C.ptr(outs.get("dtw")), len(row_off) - 1, offs, S, score_window,
                                             ws.data_ptr(), nbytes, _C.stream()), "rec_scores_signals")
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert float(b[0]) == SENT64 and float(b[-1]) == SENT64, k
    assert bool((ws[nbytes:] == 0x5a).all())
    return outs


def test_segmented_reconstruction_scores_equal_single_signal():
    from hypad_amd.utils import anomaly_detection_utils as adu
    S = 100
    # < 100 windows: smoothing window 0, all NaN; 100..199: window 1; 3 400: window 34 > 32, the chunked rolling path; 262 200 windows:
    # stat_blocks saturates at 256 slices; segment 7 reconstructs its signal exactly: every error 0, standard deviation 0
    counts = [50, 99, 100, 150, 199, 1, 3_400, 500, 700, 262_200]
    rng = np.random.default_rng(21)
    g = torch.Generator(device="cuda").manual_seed(21)
    ys, yhs, trues = [], [], []
    for k, n in enumerate(counts):
        ser = torch.from_numpy(_series(n, S, k, rng)).cuda()
        y = ser.unfold(0, S, 1).contiguous()
        assert y.shape == (n, S)
        yh = y.clone() if k == 7 else (y + 0.1 * torch.randn(n, S, device="cuda", generator=g)).contiguous()
        ys.append(y); yhs.append(yh); trues.append(ser.double())
    row_off = _offsets(counts)
    y_hat = torch.cat(yhs).contiguous()
    true = torch.cat(trues).contiguous()
    median, t_off = _unroll_signals(y_hat, row_off, S)
    assert true.numel() == t_off[-1]
    for k in range(len(counts)):
        same_bits(true[t_off[k]: t_off[k + 1]], adu.unroll_true(ys[k]), (k, "true"))
    outs = _rec_scores_signals(true, median.contiguous(), row_off, S)
    only_dtw = _rec_scores_signals(true, median.contiguous(), row_off, S, kinds=("dtw",))
    same_bits(only_dtw["dtw"], outs["dtw"], "dtw alone")
    for k, n in enumerate(counts):
        w = math.trunc(n * 0.01)
        for kind in KINDS:
            err = adu.reconstruction_errors(ys[k], yhs[k], 1, 10, w, True, kind, with_summary=False)[0]
            want = adu.zscore_clip(err)
            got = outs[kind][t_off[k]: t_off[k + 1]]
            same_bits(got, want, (k, n, kind))
            if n < 100 or k == 7:
                assert bool(torch.isnan(got).all()), (k, kind)
            else:
                assert not bool(torch.isnan(got).any()), (k, kind)


def test_other_dtw_lengths_and_windows():
    from hypad_amd.utils import anomaly_detection_utils as adu
    rng = np.random.default_rng(5)
    g = torch.Generator(device="cuda").manual_seed(5)
    for S, sw in ((48, 6), (150, 20), (100, 3)):
        counts = [120, 1, 433, 3_301, 260]
        ys = [torch.from_numpy(_series(n, S, k, rng)).cuda().unfold(0, S, 1).contiguous() for k, n in enumerate(counts)]
        yhs = [(y + 0.05 * torch.randn(y.shape, device="cuda", generator=g)).contiguous() for y in ys]
        row_off = _offsets(counts)
        true = torch.cat([adu.unroll_true(y) for y in ys]).contiguous()
        median, t_off = _unroll_signals(torch.cat(yhs).contiguous(), row_off, S)
        outs = _rec_scores_signals(true, median.contiguous(), row_off, S, score_window=sw)
        for k, n in enumerate(counts):
            for kind in KINDS:
                err = adu.reconstruction_errors(ys[k], yhs[k], 1, sw, math.trunc(n * 0.01), True, kind, with_summary=False)[0]
                same_bits(outs[kind][t_off[k]: t_off[k + 1]], adu.zscore_clip(err), (S, sw, k, kind))


def _group(counts, S, seed, dtype=np.float64):
    """Window matrices (host, `dtype`), reconstructions and critic values of a group: (x_list, res)."""
    rng = np.random.default_rng(seed)
    g = torch.Generator(device="cuda").manual_seed(seed)
    xs, yhs, crs = [], [], []
    for k, n in enumerate(counts):
        ser = _series(n, S, k, rng, dtype)
        X = np.ascontiguousarray(ser[np.arange(n)[:, None] + np.arange(S)[None, :]])[:, :, None]
        xs.append(X)
        yhs.append((torch.from_numpy(X.reshape(n, S)).cuda().float() + 0.1 * torch.randn(n, S, device="cuda", generator=g)).contiguous())
        crs.append(torch.randn(n, device="cuda", generator=g))
    res = {"recons": torch.cat(yhs).contiguous(), "eucl": None, "hyper_real": None, "critic": torch.cat(crs).contiguous(), "rowdist": None,
           "row_off": _offsets(counts)}
    return xs, res


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("comb", ["mult", "sum", "rec", "critic"])
def test_grouped_euclidean_scores_equal_score_anomalies(kind, comb):
    from hypad_amd.utils import anomaly_detection_utils as adu
    S = 100
    counts = [50, 120, 333, 1_500, 3_400]
    xs, res = _group(counts, S, seed=31)               # fp64 windows: values no fp32 series holds
    ro = res["row_off"]
    true = adu.unroll_true_signals(xs, ro, S)
    out = adu.euclidean_scores_signals(res, true, kind, comb)
    torch.cuda.synchronize()
    assert out["row_off"] == ro and out["t_off"] == adu.timestep_offsets(ro, S)
    assert sorted(out["rec_scores"]) == [kind] and (out["critic_scores"] is None) == (comb == "rec")
    for k in range(len(counts)):
        a, b, ta, tb = ro[k], ro[k + 1], out["t_off"][k], out["t_off"][k + 1]
        want = adu.score_anomalies(xs[k], res["recons"][a:b], res["critic"][a:b], None, rec_error_type=kind, comb=comb, path=None, with_true=False)[0]
        same_bits(out["final_scores"][ta:tb], torch.from_numpy(np.asarray(want)), (kind, comb, k))
        same_bits(true[ta:tb], adu.unroll_true(xs[k]), (k, "true"))
    if kind == "dtw" and comb == "mult":               # all three kinds at once: the same numbers as one at a time
        allk = adu.euclidean_scores_signals(res, true, kind, comb, kinds=KINDS)
        same_bits(allk["final_scores"], out["final_scores"], "all kinds")
        for kk in KINDS:
            same_bits(allk["rec_scores"][kk], adu.euclidean_scores_signals(res, true, kk, "rec")["final_scores"], kk)


def test_grouped_euclidean_scores_meet_the_reference_numbers():
    from hypad_amd.utils import anomaly_detection_utils as adu
    fx, fx2 = load("score.npz"), load("score_area_dtw.npz")
    S = 100
    counts = [130, 77, 300, 1_200, 410]
    xs, res = _group(counts, S, seed=41)
    ro = res["row_off"]
    xs[2] = fx["y"]
    res["recons"][ro[2]: ro[3]] = torch.from_numpy(fx["y_hat"]).cuda()
    res["critic"][ro[2]: ro[3]] = torch.from_numpy(fx["critic"]).cuda()
    true = adu.unroll_true_signals(xs, ro, S)
    t_off = adu.timestep_offsets(ro, S)
    assert maxdiff(true[t_off[2]: t_off[3]].cpu().numpy(), fx["true_unrolled"]) == 0
    for kind in KINDS:
        for comb in ("mult", "sum", "rec", "critic"):
            ref = fx.get(f"eucl_{comb}") if kind == "point" else fx2.get(f"eucl_{kind}_{comb}")
            if ref is None:
                continue
            got = adu.euclidean_scores_signals(res, true, kind, comb)["final_scores"][t_off[2]: t_off[3]].cpu().numpy()
            assert np.allclose(got, ref, rtol=0, atol=1e-6, equal_nan=True), (kind, comb, maxdiff(got, ref))


def _run_pair(tmp_path, monkeypatch, cfg, names, data, prepare=None):
    """run_signals grouped and per signal in two working directories; returns (runs, final scores seen by find_anomalies, artefacts)."""
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    seen = {}
    real_find = adu.find_anomalies

    def spy(scores, index, *a, **kw):
        seen.setdefault(key, []).append(np.array(scores, dtype=np.float64))
        return real_find(scores, index, *a, **kw)
    monkeypatch.setattr(adu, "find_anomalies", spy)
    runs, files = {}, {}
    for key, grouped in (("grouped", True), ("per_signal", False)):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        if prepare:
            prepare(wd)
        torch.manual_seed(9)
        runs[key] = hmain.run_signals(SimpleNamespace(**cfg), [n for n, _ in names], None, str(data), log=lambda s_: None, grouped_scoring=grouped)
        files[key] = artefacts(wd / "trained_models")
    monkeypatch.setattr(adu, "find_anomalies", real_find)
    return runs, seen, files


def _assert_runs_equal(runs, seen, files, names):
    from test_gpu_score_signals import _metrics
    assert len(seen["grouped"]) == len(seen["per_signal"]) == len(names)
    by_len = lambda arrs: {a.size: a for a in arrs}      # (the grouped run scores its group first: the signals differ in length)
    ga, pa = by_len(seen["grouped"]), by_len(seen["per_signal"])
    assert len(ga) == len(names) and sorted(ga) == sorted(pa)
    for n in ga:
        assert ga[n].tobytes() == pa[n].tobytes(), n
    for name, _ in names:
        ga, pa = runs["grouped"][name], runs["per_signal"][name]
        assert ga["confusion"] == pa["confusion"] and _metrics(ga) == _metrics(pa) and ga["n_intervals"] == pa["n_intervals"]
    fa, fb = files["grouped"], files["per_signal"]
    assert sorted(fa) == sorted(fb)
    for f in ("anomalies.csv", "recons_signal.pt", "critic_scores.pickle", "point.pickle", "area.pickle", "dtw.pickle"):
        assert sum(k.endswith(f) for k in fa) == len(names), f
    for k in fa:
        assert equal(fa[k], fb[k]), k


CFG = dict(dataset="NAB", signal="sa", epochs=1, hyperbolic=False, signal_shape=100, lr=5e-4, batch_size=64, save_result=False, filename="",
           rec_error="dtw", combination="mult", interval=600, unique_dataset=True, resume=False, resume_epoch=0, load=False)
NAMES = [("sa", 700), ("sb", 520), ("sc", 180)]          # 180 - 100 windows: a smoothing window of 0 (NaN scores)


@pytest.mark.parametrize("rec_error", ["point", "area"])
def test_run_signals_grouped_equals_per_signal_sum(tmp_path, monkeypatch, rec_error):
    from hypad_amd import main as hmain
    d = tmp_path / "data"
    d.mkdir()
    csv_signals(d, NAMES)
    groups = []
    real = hmain._detect_grouped
    monkeypatch.setattr(hmain, "_detect_grouped", lambda group, *a, **k: groups.append([s.name for s in group]) or real(group, *a, **k))
    runs, seen, files = _run_pair(tmp_path, monkeypatch, dict(CFG, rec_error=rec_error, combination="sum"), NAMES, d)
    assert groups == [[n for n, _ in NAMES]]           # the grouped run scored all three together, the other run none
    _assert_runs_equal(runs, seen, files, NAMES)


def test_run_signals_leaves_a_cached_signal_to_the_per_signal_detector(tmp_path, monkeypatch):
    from hypad_amd import main as hmain
    from hypad_amd import train as ht
    d = tmp_path / "data"
    d.mkdir()
    csv_signals(d, NAMES)
    # a first run tells the length of sb's scores; its dtw scores, doubled, are the cache both later runs find
    first = tmp_path / "first"
    first.mkdir()
    monkeypatch.chdir(first)
    torch.manual_seed(9)
    hmain.run_signals(SimpleNamespace(**CFG), [n for n, _ in NAMES], None, str(d), log=lambda s_: None, grouped_scoring=True)
    raw = ht.model_path(SimpleNamespace(**dict(CFG, signal="sb")))
    with open(raw + "dtw.pickle", "rb") as f:
        cached = 2.0 * np.asarray(pickle.load(f))
    assert cached.ndim == 1 and np.isfinite(cached).all()

    def prepare(wd):
        os.makedirs(os.path.dirname(raw), exist_ok=True)
        with open(raw + "dtw.pickle", "wb") as f:
            pickle.dump(cached, f, protocol=pickle.HIGHEST_PROTOCOL)
    groups = []
    real = hmain._detect_grouped
    monkeypatch.setattr(hmain, "_detect_grouped", lambda group, *a, **k: groups.append([s.name for s in group]) or real(group, *a, **k))
    runs, seen, files = _run_pair(tmp_path, monkeypatch, CFG, NAMES, d, prepare)
    assert groups == [["sa", "sc"]]
    _assert_runs_equal(runs, seen, files, NAMES)
    key = [k for k in files["grouped"] if k.endswith("sbdtw.pickle")]
    assert len(key) == 1 and files["grouped"][key[0]].tobytes() == cached.tobytes()      # read back, not rewritten
