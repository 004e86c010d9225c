"""The device interval extraction (hypad_find_anomalies_signals, utils.anomaly_detection_utils.find_anomalies_signals,
main.run_signals(device_intervals=True)) against the host find_anomalies it replaces (utils/intervals.py, pinned by
tests/golden/intervals.npz to the reference's outputs).

Contract: interval bounds equal, scores within rtol 1e-9 (the device sums in another order than NumPy's pairwise sums: about
n 2^-53 relative, 1.1e-10 at n = 10^6).  A bound can differ legitimately only when a value lies within that distance of its
window's threshold or a prune ratio within it of min_percent; every test checks on the host that its own input keeps a relative
distance > 1e-6 from both, then asserts equality."""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from helpers import csv_signals, load
from intervals_ref import RTOL, _sizes, check_precondition, host, series

pytestmark = pytest.mark.gpu


def device(segs, kw, index_list=None, seg_off=None, scores=None, **extra):
    from hypad_amd.utils import anomaly_detection_utils as adu
    if seg_off is None:
        seg_off = [0] + list(np.cumsum([len(s) for s in segs]))
        scores = np.concatenate(segs)
    kw = {k: v for k, v in kw.items() if k != "fixed_threshold"}
    return adu.find_anomalies_signals(torch.from_numpy(np.ascontiguousarray(scores)).cuda(), seg_off, index_list=index_list, **kw, **extra)


def assert_same(got, want, what=""):
    assert got.shape == want.shape, (what, got.shape, want.shape, got, want)
    assert np.array_equal(got[:, :2], want[:, :2]), (what, got, want)
    np.testing.assert_allclose(got[:, 2], want[:, 2], rtol=RTOL, atol=0, err_msg=str(what))


def _fixture_cases():
    fx = load("intervals.npz")
    cases = [c for c in json.loads(str(fx["fa_cases"])) if c["kwargs"].get("fixed_threshold")]
    assert [c["name"] for c in cases] == ["uni", "uni_edge", "whole", "nopad", "pad5_lower", "plateau", "flat", "startspike"]
    return fx, cases


def test_fixture_cases_alone():
    fx, cases = _fixture_cases()
    for c in cases:
        e, idx, ref = fx[f"fa_{c['name']}_errors"], fx[f"fa_{c['name']}_index"], fx[f"fa_{c['name']}_out"]
        check_precondition(e, c["kwargs"])
        if c["raises"]:
            assert c["raises"] == "ZeroDivisionError"
            with pytest.raises(ZeroDivisionError):
                device([e], c["kwargs"], [idx])
            continue
        assert_same(device([e], c["kwargs"], [idx])[0], ref, c["name"])


def test_fixture_cases_as_one_group():
    # every case in one call: each signal's integer window and step are passed as the arrays the C call takes; padding,
    # min_percent and lower_threshold are scalars of a call, so the cases are grouped by them -- and the group of all eight runs
    # with the detector's settings against the host function (the fixture outputs cover the per-case settings)
    fx, cases = _fixture_cases()
    by = {}
    for c in cases:
        kw = c["kwargs"]
        by.setdefault((kw.get("anomaly_padding", 50), kw.get("min_percent", 0.1), bool(kw.get("lower_threshold"))), []).append(c)
    for (pad, minp, lower), group in by.items():
        segs = [fx[f"fa_{c['name']}_errors"] for c in group]
        idx = [fx[f"fa_{c['name']}_index"] for c in group]
        sizes = [_sizes(s.size, c["kwargs"]) for s, c in zip(segs, group)]
        kw = dict(window_size=[a for a, _ in sizes], window_step_size=[b for _, b in sizes], anomaly_padding=pad, min_percent=minp,
                  lower_threshold=lower)
        if any(c["raises"] for c in group):
            with pytest.raises(ZeroDivisionError):
                device(segs, kw, idx)
            continue
        for c, got in zip(group, device(segs, kw, idx)):
            assert_same(got, fx[f"fa_{c['name']}_out"], c["name"])
    kw = dict(window_size_portion=0.33, window_step_size_portion=0.1)
    segs = [fx[f"fa_{c['name']}_errors"] for c in cases]
    for s in segs:
        check_precondition(s, kw)
    for c, s, got in zip(cases, segs, device(segs, kw)):
        assert_same(got, host(s, kw), c["name"])


def _raw(segs, kw, capacity=16, sentinel=-777.25):
    """The C call on buffers with guard words: (tables (k, capacity, 3), counts, status), every guard checked."""
    from hypad_amd import _C
    from hypad_amd.utils import anomaly_detection_utils as adu
    k = len(segs)
    off = [0] + [int(v) for v in np.cumsum([len(s) for s in segs])]
    sz = [_sizes(len(s), kw) for s in segs]
    offs, wsz, wst = _C.int64s(off), _C.int64s([a for a, _ in sz]), _C.int64s([b for _, b in sz])
    lower = int(bool(kw.get("lower_threshold")))
    scores = torch.from_numpy(np.concatenate(segs)).cuda()
    nbytes = _C.lib.hypad_find_anomalies_signals_workspace_bytes(k, offs, wsz, wst, lower)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    G = 4                                                        # guard words (fp64) around each array
    nt, ni = k * capacity * 3, (k + 1) // 2                      # counts / status: int32 pairs in fp64 words
    buf = torch.full((G + nt + G + ni + G + ni + G,), sentinel, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    p_out, p_cnt, p_st = base + 8 * G, base + 8 * (G + nt + G), base + 8 * (G + nt + G + ni + G)
    import ctypes
    _C.check(_C.lib.hypad_find_anomalies_signals(_C.ptr(scores), k, offs, wsz, wst, int(kw.get("anomaly_padding", 50)),
                                                 float(kw.get("min_percent", 0.1)), lower, ctypes.c_void_p(p_out), ctypes.c_void_p(p_cnt),
                                                 ctypes.c_void_p(p_st), capacity, ws.data_ptr(), nbytes, _C.stream()), "find_anomalies_signals")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    sent = np.float64(sentinel)
    for a in (0, G + nt, G + nt + G + ni, G + nt + G + ni + G + ni):
        assert (h[a: a + G] == sent).all(), ("guard words", a)
    tables = h[G: G + nt].reshape(k, capacity, 3).copy()
    counts = h[G + nt + G: G + nt + G + ni].copy().view(np.int32)[:k]
    status = h[G + nt + G + ni + G: G + nt + G + ni + G + ni].copy().view(np.int32)[:k]
    if k % 2:                                                    # the odd int32 behind the last signal's
        assert h[G + nt + G: G + nt + G + ni].copy().view(np.int32)[k] == sent.reshape(1).view(np.int32)[1]
    for s in range(k):                                           # no slot beyond a signal's count is written
        assert (tables[s, min(int(counts[s]), capacity):] == sent).all(), ("slots beyond the count", s)
    assert not (status & adu.FA_INTERNAL).any()
    return tables, counts, status


def _group_inputs():
    kw = dict(window_size_portion=0.33, window_step_size_portion=0.1)
    probe = series(1777, 4, 25, 101)
    others = [series(1400 + 13 * k, 2 + k % 4, 10 + k % 20, 200 + k) for k in range(69)]
    for s in [probe] + others:
        check_precondition(s, kw)
    return kw, probe, others


def test_group_independence_and_sentinels():
    kw, probe, others = _group_inputs()
    alone_t, alone_c, alone_s = _raw([probe], kw)
    assert alone_c[0] >= 1 and alone_s[0] == 0
    assert_same(alone_t[0, : alone_c[0]], host(probe, kw), "alone")
    for what, segs, at in (("first", [probe] + others[:5], 0), ("last", others[:5] + [probe], 5), ("beyond 64", others + [probe], 69),
                           ("inside 70", others[:30] + [probe] + others[30:], 30)):
        t, c, st = _raw(segs, kw)
        assert c[at] == alone_c[0] and st[at] == alone_s[0], what
        assert t[at].tobytes() == alone_t[0].tobytes(), what
        for s, seg in enumerate(segs):                           # and every other signal of the group is right
            assert st[s] == 0
            assert_same(t[s, : c[s]], host(seg, kw), (what, s))


def test_both_layouts():
    from hypad_amd.utils import anomaly_detection_utils as adu
    kw = dict(window_size_portion=0.33, window_step_size_portion=0.1)
    row_off = [0, 1500, 3100, 3400]
    t_off = adu.timestep_offsets(row_off, 100)
    assert t_off == [0, 1599, 3298, 3697]
    for off in (row_off, t_off):
        segs = [series(off[s + 1] - off[s], 3, 20, 300 + s + off[-1]) for s in range(3)]
        for s in segs:
            check_precondition(s, kw)
        idx = [np.arange(7, 7 + 5 * len(s), 5) for s in segs]
        got = device(None, kw, idx, seg_off=off, scores=np.concatenate(segs))
        assert any(len(g) for g in got)
        for s in range(3):
            assert_same(got[s], host(segs[s], kw, idx[s]), (off, s))


def test_nan_segments():
    kw = dict(window_size_portion=0.33, window_step_size_portion=0.1)
    clean = series(1600, 3, 20, 41)
    prefix = series(1600, 3, 20, 42)
    prefix[:99] = np.nan                                          # what a centred rolling mean leaves at a segment's head
    prefix[1200:1215] += 2.0
    allnan = np.full(300, np.nan)
    for s in (clean, prefix, allnan):
        check_precondition(s, kw)
    with np.errstate(invalid="ignore"):
        want = [host(s, kw) for s in (clean, prefix, allnan)]
    assert want[2].shape == (0, 3) and len(want[1]) >= 1
    got = device([clean, prefix, allnan], kw)
    for s in range(3):
        assert_same(got[s], want[s], s)
    assert_same(device([allnan], kw)[0], want[2], "all NaN alone")


@pytest.mark.parametrize("n,kw,seed", [(1_000_000, dict(window_size_portion=0.33, window_step_size_portion=0.1), 7),
                                       (125_000, dict(window_size_portion=0.2, window_step_size_portion=0.1, anomaly_padding=200), 8)])
def test_scale(n, kw, seed):
    e = series(n, 40, 300, seed)
    check_precondition(e, kw)
    want = host(e, kw)
    assert len(want) >= 3
    assert_same(device([e], kw)[0], want, n)


def test_more_runs_than_an_lds_sort_holds():
    # padding 0, 5 000 two-point spikes in a 400 000-point window: more runs than the 4 096 keys of the LDS sort, and more kept rows
    # per signal; every run has weight stop - start = 1, so no merge group has zero weight
    n = 450_000
    e = 1.0 + 0.1 * np.abs(np.random.default_rng(12).standard_normal(n))
    for c in range(40, n - 2, 80):
        e[c: c + 2] += 2.0
    kw = dict(window_size=400_000, window_step_size=50_000, anomaly_padding=0)
    check_precondition(e, kw)
    want = host(e, kw)
    assert len(want) > 4096
    assert_same(device([e], kw)[0], want, "pad 0")


def test_capacity_overflow_is_reported_and_nothing_is_written_out_of_bounds():
    from hypad_amd.utils import anomaly_detection_utils as adu
    kw = dict(window_size_portion=0.33, window_step_size_portion=0.1, anomaly_padding=5)
    many = series(3000, 30, 6, 55)
    few = series(1500, 1, 10, 56)
    for s in (many, few):
        check_precondition(s, kw)
    want = [host(many, kw), host(few, kw)]
    assert len(want[0]) > 4 >= len(want[1])
    t, c, st = _raw([many, few], kw, capacity=4)                  # (_raw checks the guard words and the slots beyond the counts)
    assert c[0] == len(want[0]) and st[0] == adu.FA_OVERFLOW
    assert c[1] == len(want[1]) and st[1] == 0
    assert_same(t[0], want[0][:4], "the first rows of the overflowing table")
    assert_same(t[1, : c[1]], want[1], "its neighbour")
    got = device([many, few], kw, capacity=4)                     # the mirror asks again with room for the largest count
    assert_same(got[0], want[0], "retried")
    assert_same(got[1], want[1], "retried")


def _anomaly_files(root):
    import pandas as pd
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith("anomalies.csv"):
                out[os.path.relpath(os.path.join(dirpath, f), root)] = pd.read_csv(os.path.join(dirpath, f), index_col=0).to_numpy(dtype=np.float64)
    return out


@pytest.mark.parametrize("hyperbolic", [True, False])
def test_run_signals_device_intervals(tmp_path, monkeypatch, hyperbolic):
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    d = tmp_path / "data"
    d.mkdir()
    names = [("sa", 400), ("sb", 300)]
    csv_signals(d, names)
    cfg = dict(dataset="NAB", signal="sa", epochs=1, hyperbolic=hyperbolic, signal_shape=100, lr=5e-4, batch_size=64, save_result=False,
               filename="", rec_error="dtw", combination="mult", interval=600, unique_dataset=True, resume=False, resume_epoch=0, load=False)
    seen = []
    real_find = adu.find_anomalies

    def spy(scores, index, *a, **kw):
        seen.append(np.array(scores, dtype=np.float64))
        return real_find(scores, index, *a, **kw)
    monkeypatch.setattr(adu, "find_anomalies", spy)
    runs = {}
    for key, dev in (("host", False), ("device", True)):
        wd = tmp_path / key
        wd.mkdir()
        monkeypatch.chdir(wd)
        torch.manual_seed(9)
        runs[key] = hmain.run_signals(SimpleNamespace(**cfg), [n for n, _ in names], None, str(d), log=lambda s_: None, device_intervals=dev)
    assert len(seen) == len(names)                                # the host run's calls only: the device run skips find_anomalies
    for scores in seen:
        check_precondition(scores, dict(window_size_portion=0.33, window_step_size_portion=0.1))
    for name, _ in names:
        a, b = runs["host"][name], runs["device"][name]
        assert a["confusion"] == b["confusion"] and a["n_intervals"] == b["n_intervals"], name
    fa, fb = _anomaly_files(tmp_path / "host" / "trained_models"), _anomaly_files(tmp_path / "device" / "trained_models")
    assert sorted(fa) == sorted(fb) and len(fa) == len(names)
    for k in fa:
        assert_same(fb[k].reshape(-1, 3), fa[k].reshape(-1, 3), k)


def test_cli_device_intervals_flag(tmp_path, monkeypatch):
    import yaml
    from hypad_amd import main as hmain
    from hypad_amd.utils import anomaly_detection_utils as adu
    d = tmp_path / "data"
    d.mkdir()
    csv_signals(d, [("sa", 400), ("sb", 300)])
    cfg = dict(dataset="NAB", signal="sa", epochs=1, hyperbolic=True, signal_shape=100, lr=5e-4, batch_size=64, save_result=False, filename="",
               rec_error="dtw", combination="mult", interval=600, unique_dataset=True, resume=False, resume_epoch=0, load=False)
    with open(tmp_path / "cfg.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    called = []
    real = adu.find_anomalies_signals
    monkeypatch.setattr(adu, "find_anomalies_signals", lambda *a, **k: called.append(1) or real(*a, **k))
    monkeypatch.chdir(tmp_path)
    out = {}
    for flag in ([], ["--device-intervals"]):
        torch.manual_seed(9)
        out[bool(flag)] = hmain.main(["--config", str(tmp_path / "cfg.yaml"), "--data-dir", str(d), "--signals", "sa,sb"] + flag)
    assert called == [1]                                          # off by default
    assert {k: (v["confusion"], v["n_intervals"]) for k, v in out[False].items()} == {k: (v["confusion"], v["n_intervals"]) for k, v in out[True].items()}
    for bad in (["--device-intervals", "--per-signal-scoring"],):
        with pytest.raises(SystemExit):
            hmain.main(["--config", str(tmp_path / "cfg.yaml"), "--data-dir", str(d), "--signals", "sa,sb"] + bad)
