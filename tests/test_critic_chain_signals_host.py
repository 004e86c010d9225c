"""CPU-only checks of the segmented critic-score chain (hypad_quantiles_signals, hypad_critic_chain_signals): the new entry points are
declared in include/hypad.h, exported and bound; their argument errors come back with the documented codes before anything is
launched (no GPU needed); the workspace sizes grow with the group and are what the calls insist on."""
import ctypes
import os
import re

import pytest

from hypad_amd import _C
from hypad_amd.utils import anomaly_detection_utils as adu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hypad_quantiles_signals_workspace_bytes", "hypad_quantiles_signals", "hypad_critic_chain_signals_workspace_bytes",
       "hypad_critic_chain_signals")
EINVAL, EWORKSPACE, EUNSUPPORTED = -1, -2, -3
BIG = 1 << 40


def _p(v=256):
    return ctypes.c_void_p(v)


def _ptr(v):
    return None if v is None else _p(v)


def _q(values):
    return (ctypes.c_double * max(len(values), 1))(*values)


def _quant(src=256, off=(0, 4, 9), n=None, window=100, q=(0.25, 0.75), nq=None, out=256, ws=256, ws_bytes=BIG, q_null=False):
    n = len(off) - 1 if n is None else n
    return _C.lib.hypad_quantiles_signals(_ptr(src), n, _C.int64s(off) if off is not None else None, window, None if q_null else _q(q),
                                          len(q) if nq is None else nq, _ptr(out), _ptr(ws), ws_bytes, None)


def _chain(critic=256, modes=None, out=256, off=(0, 4, 9), n=None, window=100, ws=256, ws_bytes=BIG):
    n = len(off) - 1 if n is None else n
    return _C.lib.hypad_critic_chain_signals(_ptr(critic), _ptr(modes), _ptr(out), n, _C.int64s(off) if off is not None else None, window,
                                             _ptr(ws), ws_bytes, None)


def test_new_entry_points_are_declared_exported_and_bound():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hypad.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hypad_[a-z0-9_]+)\s*\(", header))
    for name in NEW:
        assert name in declared, name
        assert name in _C.EXPORTS and hasattr(_C.lib, name), name
    assert _C.lib.hypad_abi_version() == 7 and re.search(r"#define HYPAD_ABI_VERSION 7\b", open(os.path.join(ROOT, "include", "hypad.h")).read())
    assert callable(adu.final_critic_scores_signals)


def test_declarations_cite_the_reference_lines_they_replace():
    header = open(os.path.join(ROOT, "include", "hypad.h")).read()
    for name in ("hypad_quantiles_signals_workspace_bytes", "hypad_critic_chain_signals_workspace_bytes"):
        comment = header[:header.index("size_t " + name)].rsplit("/*", 1)[1]
        assert re.search(r":\d+-\d+", comment), name


@pytest.mark.parametrize("off", [[0, 5, 3], [0, 5, 5, 9], [2, 5, 9], [0]])
def test_bad_offsets_are_rejected_without_a_launch(off):
    # (row_off[0] != 0, an empty signal, descending offsets, no signal at all)
    assert _quant(off=off) == EINVAL
    assert _chain(off=off) == EINVAL
    assert _C.lib.hypad_critic_chain_signals_workspace_bytes(len(off) - 1, _C.int64s(off), 100) == 0


def test_quantiles_signals_argument_errors():
    assert _quant(src=None) == EINVAL and _quant(out=None) == EINVAL and _quant(q_null=True) == EINVAL
    assert _quant(off=None, n=2) == EINVAL
    assert _quant(window=0) == EINVAL and _quant(window=-3) == EINVAL
    assert _quant(q=(), nq=0) == EINVAL
    assert _quant(q=(0.1, 0.5, 0.9)) == EUNSUPPORTED                        # nq = 3, as hypad_quantiles
    for bad in ((-0.01, 0.5), (0.5, 1.01), (float("nan"),)):
        assert _quant(q=bad) == EINVAL, bad
    assert _quant(off=(0, 4, (1 << 31) + 9), window=1) == EUNSUPPORTED       # a segment beyond hypad_quantiles' 2^31 values
    need = _C.lib.hypad_quantiles_signals_workspace_bytes(2)
    assert need > 0
    assert _quant(ws_bytes=need - 1) == EWORKSPACE and _quant(ws=None) == EWORKSPACE
    assert _C.lib.hypad_quantiles_signals_workspace_bytes(0) == 0 and _C.lib.hypad_quantiles_signals_workspace_bytes(-1) == 0


def test_critic_chain_signals_argument_errors():
    assert _chain(critic=None) == EINVAL and _chain(out=None) == EINVAL
    assert _chain(off=None, n=2) == EINVAL
    assert _chain(window=0) == EINVAL and _chain(window=-1) == EINVAL
    assert _chain(window=257) == EUNSUPPORTED                                # beyond the KDE kernel's window limit, as hypad_kde_mode
    off = _C.int64s([0, 4, 9])
    need = _C.lib.hypad_critic_chain_signals_workspace_bytes(2, off, 100)
    assert need > 0
    assert _chain(ws_bytes=need - 1) == EWORKSPACE and _chain(ws=None) == EWORKSPACE
    assert _chain(modes=256, ws_bytes=need - 1) == EWORKSPACE
    assert _C.lib.hypad_critic_chain_signals_workspace_bytes(2, off, 0) == 0
    assert _C.lib.hypad_critic_chain_signals_workspace_bytes(2, None, 100) == 0
    for rc in (EINVAL, EWORKSPACE, EUNSUPPORTED):
        with pytest.raises(_C.HypadError):
            _C.check(rc, "critic_chain_signals")


def test_workspaces_are_monotone_in_the_number_of_signals():
    qws = _C.lib.hypad_quantiles_signals_workspace_bytes
    sizes = [qws(n) for n in range(1, 200)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[1] > sizes[0] and sizes[63] > sizes[31]                      # a slice per segment of a launch ...
    assert sizes[63] == sizes[64] == sizes[198]                               # ... and the chunks of a larger group share them
    # one slice holds the three global histograms (4 ranks x 2 048 bins) and four candidate lists of 4 096 keys
    assert sizes[0] >= 3 * 4 * 2048 * 4 + 4 * 4096 * 8
    cws = _C.lib.hypad_critic_chain_signals_workspace_bytes
    prev = 0
    for n in (1, 2, 5, 32, 64, 65, 70, 130):
        off = [0]
        for k in range(n):
            off.append(off[-1] + 1 + 37 * (k % 5))
        got = cws(n, _C.int64s(off), 100)
        total = off[-1] + n * 99
        # the quantile slices + the unsmoothed scores and the modes in timestep layout
        assert got >= qws(n) + 2 * 8 * total
        assert got > prev
        prev = got
        # what the call insists on is what the function says: one byte less is refused, for any group size
        assert _chain(off=off, ws_bytes=got - 1) == EWORKSPACE
        assert _quant(off=off, ws_bytes=qws(n) - 1) == EWORKSPACE


def test_mirror_refuses_a_critic_vector_that_does_not_match_the_offsets():
    import torch
    with pytest.raises(ValueError, match="offsets say 9 windows"):
        adu.final_critic_scores_signals(torch.zeros(8), [0, 4, 9], 100)
