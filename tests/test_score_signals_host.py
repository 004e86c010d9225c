"""CPU-only checks of the signal-group scoring entry points: offsets, the forward launch's tile plan, and argument checks that
return HYPAD_EINVAL before anything is launched (no GPU needed)."""
import ctypes

import pytest

from hypad_amd import _C
from hypad_amd import anomaly_detection as ad

BAD = [
    ("non-monotonic", [0, 5, 3]),
    ("empty segment", [0, 5, 5, 9]),
    ("not from 0", [2, 5, 9]),
]


def test_signal_offsets():
    assert ad.signal_offsets([1, 15, 16]) == [0, 1, 16, 32]
    with pytest.raises(ValueError):
        ad.signal_offsets([4, 0, 2])


def test_tile_plan_follows_the_total_and_never_straddles_signals():
    # the reference shape takes 32-window tiles from 65 536 windows in the group on, as hypad_score_forward_packed does from its rows
    assert ad.tile_plan([0, 1, 16, 33], 100, 20) == (16, 1 + 1 + 2)
    off = ad.signal_offsets([1, 15, 16, 17, 33, 65_541])
    assert ad.tile_plan(off, 100, 20) == (32, 1 + 1 + 1 + 1 + 2 + 2049)
    assert ad.tile_plan(off, 150, 20) == (16, 1 + 1 + 1 + 2 + 3 + 4097)
    assert ad.tile_plan([0, 65_535], 100, 20) == (16, 4096)
    assert ad.tile_plan([0, 65_536], 100, 20) == (32, 2048)


def test_workspace_grows_with_the_group():
    one = _C.lib.hypad_score_signals_workspace_bytes(100, 20, 1, 1)
    assert one >= _C.lib.hypad_score_workspace_bytes(100, 20, 1) and one % 256 == 0
    assert _C.lib.hypad_score_signals_workspace_bytes(100, 20, 1, 40) == 40 * one
    assert _C.lib.hypad_score_signals_workspace_bytes(100, 20, 1, 0) == 0
    off = _C.int64s([0, 50, 1050])
    assert _C.lib.hypad_critic_score_signals_workspace_bytes(2, off, 100) >= (1050 + 2 * 99) * 8 + _C.lib.hypad_critic_score_workspace_bytes()
    assert _C.lib.hypad_critic_score_signals_workspace_bytes(2, _C.int64s([0, 5, 5]), 100) == 0


def _calls(row_off, n):
    """Every new entry point with these offsets and (fake, never dereferenced) device pointers."""
    p = ctypes.c_void_p(256)
    off, xoff = _C.int64s(row_off), _C.int64s([0] * max(n, 1))
    ws = ctypes.c_void_p(4096)
    return {
        "score_forward_signals": lambda: _C.lib.hypad_score_forward_signals(p, p, p, n, off, xoff, p, 1, p, p, p, p, p, 100, 20, 1, ws, 1 << 30, None),
        "score_signals_tiles": lambda: _C.lib.hypad_score_signals_tiles(100, 20, n, off, None, None),
        "kde_mode_signals": lambda: _C.lib.hypad_kde_mode_signals(p, p, n, off, 100, None),
        "critic_score_signals": lambda: _C.lib.hypad_critic_score_signals(p, p, n, off, 100, ws, 1 << 30, None),
        "combine_signals": lambda: _C.lib.hypad_combine_scores_signals(1, p, p, None, p, n, off, 100, None),
    }


@pytest.mark.parametrize("what,row_off", BAD)
def test_bad_offsets_are_rejected_without_a_launch(what, row_off):
    for name, call in _calls(row_off, len(row_off) - 1).items():
        with pytest.raises(_C.HypadError, match="invalid|-1"):
            _C.check(call(), name)


def test_no_signals_is_rejected():
    for name, call in _calls([0], 0).items():
        with pytest.raises(_C.HypadError):
            _C.check(call(), name)


def test_other_bad_arguments():
    p = ctypes.c_void_p(256)
    off = _C.int64s([0, 4, 9])
    # a negative x offset, a critic output without critic weights, a workspace too small
    rc = _C.lib.hypad_score_forward_signals(p, p, p, 2, off, _C.int64s([0, -1]), p, 1, p, p, p, p, p, 100, 20, 1, p, 1 << 30, None)
    assert rc == -1
    rc = _C.lib.hypad_score_forward_signals(p, p, None, 2, off, _C.int64s([0, 4]), p, 1, p, p, p, p, p, 100, 20, 1, p, 1 << 30, None)
    assert rc == -1
    rc = _C.lib.hypad_score_forward_signals(p, p, p, 2, off, _C.int64s([0, 4]), p, 1, p, p, p, p, p, 100, 20, 1, p, 64, None)
    assert rc == -2
    assert _C.lib.hypad_combine_scores_signals(42, p, p, None, p, 2, off, 100, None) == -1
    assert _C.lib.hypad_kde_mode_signals(p, p, 2, off, 0, None) == -1
