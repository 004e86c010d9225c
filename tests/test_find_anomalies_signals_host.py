"""CPU-only checks of the device interval extraction (hypad_find_anomalies_signals): the entry points are declared in include/hypad.h,
exported and bound, their comment cites the reference lines they replace, every argument error comes back with its code before
anything is launched (no GPU needed), the workspace grows with the group, the mirror refuses the dynamic threshold, and
detect_intervals(intervals=...) gives what the default path gives."""
import ctypes
import os
import re

import numpy as np
import pytest

from hypad_amd import _C
from hypad_amd.utils import anomaly_detection_utils as adu
from hypad_amd.utils import intervals as iv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hypad_find_anomalies_signals_workspace_bytes", "hypad_find_anomalies_signals")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
BIG = 1 << 50


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _arr(v):
    return None if v is None else _C.int64s(v)


def _call(scores=256, off=(0, 700, 1500), n=None, size=(231, 264), step=(24, 27), pad=50, min_percent=0.1, lower=0, out=256, counts=256,
          status=256, capacity=8, ws=256, ws_bytes=BIG):
    n = len(off) - 1 if n is None else n
    return _C.lib.hypad_find_anomalies_signals(_ptr(scores), n, _arr(off), _arr(size), _arr(step), pad, min_percent, lower, _ptr(out),
                                               _ptr(counts), _ptr(status), capacity, _ptr(ws), ws_bytes, None)


def _bytes(off, size, step, lower=0, n=None):
    n = len(off) - 1 if n is None else n
    return _C.lib.hypad_find_anomalies_signals_workspace_bytes(n, _arr(off), _arr(size), _arr(step), lower)


def test_new_entry_points_are_declared_exported_and_bound():
    text = open(os.path.join(ROOT, "include", "hypad.h")).read()
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    for name in NEW:
        assert name in declared, name
        assert name in _C.EXPORTS and hasattr(_C.lib, name), name
    assert _C.lib.hypad_abi_version() == 7 and re.search(r"#define HYPAD_ABI_VERSION 7\b", text)
    for name, value in (("HYPAD_FA_ZERO_WEIGHT", adu.FA_ZERO_WEIGHT), ("HYPAD_FA_OVERFLOW", adu.FA_OVERFLOW), ("HYPAD_FA_INTERNAL", adu.FA_INTERNAL)):
        assert re.search(r"#define %s %d\b" % (name, value), text), name
    assert callable(adu.find_anomalies_signals)


def test_declaration_cites_the_reference_lines_it_replaces():
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    comment = header[:header.index("size_t hypad_find_anomalies_signals_workspace_bytes")].rsplit("/*", 4)[1]
    for lines in (":1363-1472", ":1098-1114", ":1117-1313"):
        assert lines in comment, lines
    assert header.index("Signal groups") < header.index("hypad_find_anomalies_signals")


@pytest.mark.parametrize("off", [[0, 5, 3], [0, 5, 5, 9], [2, 5, 9], [0]])
def test_bad_offsets_are_rejected_without_a_launch(off):
    k = max(len(off) - 1, 1)
    assert _call(off=off, size=[3] * k, step=[1] * k) == EINVAL
    assert _bytes(off, [3] * k, [1] * k) == 0


def test_argument_errors():
    for name in ("scores", "out", "counts", "status"):
        assert _call(**{name: None}) == EINVAL, name
    assert _call(off=None, n=2) == EINVAL and _call(size=None) == EINVAL and _call(step=None) == EINVAL
    assert _call(size=(0, 264)) == EINVAL and _call(size=(231, -4)) == EINVAL        # window_size < 1
    assert _call(step=(24, 0)) == EINVAL and _call(step=(-1, 27)) == EINVAL          # step < 1
    assert _call(pad=-1) == EINVAL
    assert _call(capacity=0) == EINVAL
    assert _call(off=(0, 1 << 31), size=(5,), step=(5,)) == EUNSUPPORTED             # positions are 32-bit
    need = _bytes((0, 700, 1500), (231, 264), (24, 27))
    assert need > 0
    assert _call(ws_bytes=need - 1) == EWORKSPACE and _call(ws=None) == EWORKSPACE
    need2 = _bytes((0, 700, 1500), (231, 264), (24, 27), lower=1)
    assert need2 > need and _call(lower=1, ws_bytes=need2 - 1) == EWORKSPACE          # the mirrored pass has items of its own
    assert _bytes((0, 700, 1500), (231, 0), (24, 27)) == 0 and _bytes((0, 700, 1500), (231, 264), (0, 27)) == 0
    assert _bytes((0, 700, 1500), None, (24, 27)) == 0 and _bytes(None, (231, 264), (24, 27), n=2) == 0
    for rc in (EINVAL, EWORKSPACE, EUNSUPPORTED):
        with pytest.raises(_C.HypadError):
            _C.check(rc, "find_anomalies_signals")


def test_unsupported_sizes_are_refused_by_the_bytes_function_and_by_the_call():
    # a segment beyond 32-bit positions, and a window of more than 65 535 reduction chunks (the grid's y extent): no workspace size
    # (nothing to allocate), HYPAD_EUNSUPPORTED from the call before any launch
    chunk = 4096
    for off, size, step in (((0, (1 << 31)), (5,), (5,)), ((0, 700, 700 + (1 << 31)), (231, 5), (24, 5)),
                            ((0, 65536 * chunk), (65536 * chunk,), (chunk,)), ((0, 65536 * chunk + 9), (65535 * chunk + 1,), (7,))):
        for lower in (0, 1):
            assert _bytes(off, size, step, lower) == 0
            assert _call(off=off, size=size, step=step, lower=lower) == EUNSUPPORTED
    assert _bytes((0, (1 << 31) - 1), (5,), (1 << 30,)) > 0                           # INT_MAX values are positions still
    assert _bytes((0, 65536 * chunk), (65535 * chunk,), (65535 * chunk,)) > 0        # 65 535 chunks are a grid still
    assert _call(capacity=-3) == EINVAL and _call(pad=-(1 << 40)) == EINVAL           # (beside capacity 0 and padding -1 above)


def test_workspace_grows_with_the_group():
    prev = 0
    for n in (1, 2, 5, 32, 64, 65, 70, 130):
        off, size, step = [0], [], []
        for k in range(n):
            t = 1400 + 37 * (k % 17)
            off.append(off[-1] + t)
            size.append(int(np.ceil(t * 0.33)))
            step.append(int(np.ceil(size[-1] * 0.1)))
        got = _bytes(off, size, step)
        assert got > prev
        prev = got
        # four partial sums per window and chunk at the least
        windows = sum(-(-(o1 - o0 - sz) // st) + 1 for o0, o1, sz, st in zip(off, off[1:], size, step))
        assert got >= windows * 4 * 8
        # what the call insists on is what the function says
        assert _call(off=off, size=size, step=step, ws_bytes=got - 1) == EWORKSPACE
    one = _bytes((0, 1_000_000), (330_000,), (33_000,))
    assert one > _bytes((0, 125_000), (41_250,), (4_125,)) > 0


def test_mirror_refuses_the_dynamic_threshold_before_touching_the_device():
    with pytest.raises(ValueError, match="fixed"):
        adu.find_anomalies_signals(np.ones(10), [0, 10], fixed_threshold=False)
    with pytest.raises(ValueError, match="fixed"):
        adu.find_anomalies_signals(np.ones(10), [0, 10], fixed_threshold=None)


def test_detect_intervals_takes_given_intervals():
    from types import SimpleNamespace
    rng = np.random.default_rng(3)
    e = 1.0 + 0.1 * np.abs(rng.standard_normal(1500))
    e[400:420] += 2.0
    e[1100:1108] += 1.5
    index = np.arange(5000, 5000 + 3 * e.size, 3)
    known = [(index[395], index[425]), (index[30], index[40])]
    params = SimpleNamespace(save_result=False)
    want = adu.detect_intervals(e, params, None, index, known, "s")
    assert want["intervals"].shape[0] >= 1
    given = iv.find_anomalies(e, index, window_size_portion=0.33, window_step_size_portion=0.1, fixed_threshold=True)
    calls = []
    real = adu.find_anomalies
    adu.find_anomalies = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        got = adu.detect_intervals(e, params, None, index, known, "s", intervals=given)
    finally:
        adu.find_anomalies = real
    assert calls == []                                           # find_anomalies is skipped
    assert sorted(got) == sorted(want)
    assert got["intervals"].tobytes() == want["intervals"].tobytes() and got["final_scores"].tobytes() == want["final_scores"].tobytes()
    assert got["confusion"] == want["confusion"] and repr(got["metrics"]) == repr(want["metrics"])
    empty = adu.detect_intervals(e, params, None, index, known, "s", intervals=np.zeros((0, 3)))
    assert empty["intervals"].shape == (0, 3) and empty["confusion"] == [0, 0, 0, 0] and empty["metrics"] is None
