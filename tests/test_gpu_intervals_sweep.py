"""The interval-extraction kernels (csrc/intervals.hip: fa_reduce_kernel<0|1|2>, fa_window_kernel, fa_merge_kernel with block_scan and
bitonic_sort) against the host find_anomalies at their launch edges: window lengths around the 1 024-thread tile and the 4 096-element
reduction chunk, values above the threshold on tile and mask-word seams, paddings longer than a tile and than a window, run gaps of
2 pad, 2 pad + 1 and 2 pad + 2, 4 095 / 4 096 / 4 097 keys on either side of the LDS sort in the run sort and in the merge sort, the
densest window the cap allows, empty and degenerate items, groups that mix all of it across the 64-signal launch chunks, ties, signs,
and the covered window whose sentinel row the reference keeps.

Everything goes through the C entry point.  The workspace has exactly the size hypad_find_anomalies_signals_workspace_bytes returns, is
filled with a byte pattern and followed by a guard; tables, counts and status sit between sentinels; HYPAD_FA_INTERNAL must never be
set.  Interval bounds are compared with ==, scores within the allowance derived in tests/intervals_ref.py (below the contract's
rtol 1e-9, asserted on the CPU by tests/test_intervals_reference.py), the unmerged rows of the integer-valued families as bits.
The inputs, their properties and the precondition that makes equality of the bounds a fair demand are built and asserted on the CPU
(tests/intervals_ref.py, tests/test_intervals_reference.py).  Each test prints its worst error / allowance; the measured values, the
derivation and the mutation check are in docs/history/intervals_sweep.md.
"""
import ctypes

import numpy as np
import pytest
import torch

import intervals_ref as R

pytestmark = pytest.mark.gpu

GUARD = 4096                                                     # bytes behind the workspace
SENTINEL = -777.25


def raw(segs, kw, capacity, fill=0xA5):
    """The C call: (tables (k, capacity, 3), counts, status).  Workspace of exactly the returned size, pre-filled with `fill`, with a guard
    behind it; output arrays between sentinel words; every guard checked, no slot beyond a signal's count written, FA_INTERNAL unset."""
    from hypad_amd import _C
    from hypad_amd.utils import anomaly_detection_utils as adu
    k = len(segs)
    off = [0] + [int(v) for v in np.cumsum([len(s) for s in segs])]
    offs, wsz, wst = _C.int64s(off), _C.int64s(kw["window_size"]), _C.int64s(kw["window_step_size"])
    lower = int(bool(kw["lower_threshold"]))
    scores = torch.from_numpy(np.concatenate(segs)).cuda()
    nbytes = _C.lib.hypad_find_anomalies_signals_workspace_bytes(k, offs, wsz, wst, lower)
    assert nbytes == R.workspace_bytes([len(s) for s in segs], kw["window_size"], kw["window_step_size"], lower)
    ws = torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
    ws[nbytes:] = 0x3C
    G = 4                                                        # guard words (fp64) around each array
    nt, ni = k * capacity * 3, (k + 1) // 2                      # counts / status: int32 pairs in fp64 words
    buf = torch.full((G + nt + G + ni + G + ni + G,), SENTINEL, dtype=torch.float64, device="cuda")
    base = buf.data_ptr()
    p_out, p_cnt, p_st = base + 8 * G, base + 8 * (G + nt + G), base + 8 * (G + nt + G + ni + G)
    _C.check(_C.lib.hypad_find_anomalies_signals(_C.ptr(scores), k, offs, wsz, wst, int(kw["anomaly_padding"]), float(kw["min_percent"]), lower,
                                                 ctypes.c_void_p(p_out), ctypes.c_void_p(p_cnt), ctypes.c_void_p(p_st), capacity, ws.data_ptr(),
                                                 nbytes, _C.stream()), "find_anomalies_signals")
    torch.cuda.synchronize()
    assert (ws[nbytes:] == 0x3C).all().item(), "the guard behind the workspace"
    h = buf.cpu().numpy()
    sent = np.float64(SENTINEL)
    for a in (0, G + nt, G + nt + G + ni, G + nt + G + ni + G + ni):
        assert (h[a: a + G] == sent).all(), ("guard words", a)
    tables = h[G: G + nt].reshape(k, capacity, 3).copy()
    counts = h[G + nt + G: G + nt + G + ni].copy().view(np.int32)[:k]
    status = h[G + nt + G + ni + G: G + nt + G + ni + G + ni].copy().view(np.int32)[:k]
    if k % 2:                                                    # the odd int32 behind the last signal's
        for a in (G + nt + G, G + nt + G + ni + G):
            assert h[a: a + ni].copy().view(np.int32)[k] == sent.reshape(1).view(np.int32)[1]
    for s in range(k):                                           # no slot beyond a signal's count is written
        assert (tables[s, min(int(counts[s]), capacity):] == sent).all(), ("slots beyond the count", s)
    assert not (status & adu.FA_INTERNAL).any(), ("FA_INTERNAL", np.flatnonzero(status & adu.FA_INTERNAL))
    return tables, counts, status


def positions(rows, n):
    """Table positions as the reference reports them: looked up in the index 0 .. n - 1, where the sentinel row's -1 is index[-1]."""
    p = rows.astype(np.int64)
    assert (p == rows).all() and (p >= -1).all() and (p < n).all(), rows
    assert ((p[:, 0] == -1) == (p[:, 1] == -1)).all() and (p[1:] >= 0).all(), rows      # only a first window's sentinel row
    return np.arange(n)[p]


def compare(got, seg, ref, exact, what):
    """Bounds equal, scores within the allowance (bits for the unmerged rows of an integer-valued input): worst error / allowance."""
    want, allowance, merged = ref
    assert got.shape == want.shape, (what, got.shape, want.shape, got, want)
    if not len(want):
        return 0.0
    assert np.array_equal(positions(got[:, :2], len(seg)), want[:, :2]), (what, got, want)
    err = np.abs(got[:, 2] - want[:, 2])
    if exact:
        same = got[:, 2].copy().view(np.int64) == want[:, 2].copy().view(np.int64)
        assert same[~merged].all(), (what, "bits of unmerged rows", got[~merged & ~same], want[~merged & ~same])
        err, allowance = err[merged], allowance[merged]
        if not len(err):
            return 0.0
    assert np.isfinite(got[:, 2]).all() and (allowance > 0).all(), what
    ratio = err / allowance
    assert (ratio <= 1.0).all(), (what, "error / allowance", ratio.max(), got[:, 2], want[:, 2])
    return float(ratio.max())


def references(segs, kw):
    """Per segment (table, allowance, merged), or ZeroDivisionError where the host raises it."""
    out = []
    for s, e in enumerate(segs):
        try:
            out.append(R.reference(e, R.signal_kw(kw, s)))
        except ZeroDivisionError as exc:
            out.append(exc)
    return out


def run_call(name, segs, kw, exact, refs=None, second_pattern=False):
    """One C call against the host, signal by signal; (worst error / allowance, tables, counts, status)."""
    from hypad_amd.utils import anomaly_detection_utils as adu
    refs = references(segs, kw) if refs is None else refs
    capacity = max([len(r[0]) for r in refs if not isinstance(r, Exception)] + [8]) + 1
    tables, counts, status = raw(segs, kw, capacity)
    worst = 0.0
    for s, (seg, ref) in enumerate(zip(segs, refs)):
        if isinstance(ref, Exception):                           # touching zero-length sequences: the reference raises, the call flags
            assert status[s] & adu.FA_ZERO_WEIGHT, (name, s)
            continue
        assert status[s] == 0 and counts[s] == len(ref[0]), (name, s, status[s], counts[s], len(ref[0]))
        worst = max(worst, compare(tables[s, : counts[s]], seg, ref, exact, (name, s)))
    if second_pattern:                                           # nothing may depend on what the workspace held
        t2, c2, s2 = raw(segs, kw, capacity, fill=0x5A)
        assert t2.tobytes() == tables.tobytes() and c2.tobytes() == counts.tobytes() and s2.tobytes() == status.tobytes(), name
    return worst, tables, counts, status


def run_family(calls, exact=False):
    worst = 0.0
    for i, (name, segs, kw) in enumerate(calls):
        worst = max(worst, run_call(name, segs, kw, exact, second_pattern=i == 0)[0])
    print(f"worst error / allowance: {worst:.3f}" if not exact else f"unmerged rows: exact bits; merged rows, worst error / allowance: {worst:.3f}")
    return worst


@pytest.mark.parametrize("pad", R.TILE_PADS)
def test_tile_and_chunk_lengths(pad):
    run_family(R.family_tile_lengths(pad))


@pytest.mark.parametrize("first", R.TILE_OFFSETS)
def test_tile_lengths_at_a_segment_offset(first):
    run_family(R.family_tile_offsets(first))


@pytest.mark.parametrize("pad", R.GAP_PADS)
def test_run_gap_edges(pad):
    run_family(R.family_run_gaps(pad))


@pytest.mark.parametrize("count", R.SORT_COUNTS)
def test_run_sort_on_both_sides_of_the_lds_sort(count):
    run_family(R.family_sort_runs(count))


@pytest.mark.parametrize("rows", (4096, 4097))
def test_merge_sort_on_both_sides_of_the_lds_sort(rows):
    run_family(R.family_sort_merge(rows))


def test_the_cap_and_the_exact_tie():
    run_family(R.family_cap(), exact=True)


@pytest.mark.parametrize("lower", (False, True))
def test_empty_and_degenerate_items(lower):
    run_family(R.family_degenerate(lower))


@pytest.mark.parametrize("total", (65, 129))
def test_mixed_group_equals_every_signal_alone(total):
    (name, segs, kw), = R.family_mixed(total)
    refs = references(segs, kw)
    worst, tables, counts, status = run_call(name, segs, kw, False, refs=refs, second_pattern=True)
    capacity = tables.shape[1]
    for s, seg in enumerate(segs):
        kw1 = dict(kw, window_size=[kw["window_size"][s]], window_step_size=[kw["window_step_size"][s]])
        t, c, st = raw([seg], kw1, capacity)
        assert c[0] == counts[s] and st[0] == status[s], (name, s)
        assert t[0].tobytes() == tables[s].tobytes(), (name, s)
    print(f"worst error / allowance: {worst:.3f}")


def test_signs_and_ties():
    run_family(R.family_signs_and_ties(), exact=True)


def test_values_on_the_rim_of_a_run_and_across_the_tile_seam_stay_inside_it():
    run_family(R.family_shoulders())


def test_merge_carries_the_largest_stop_across_a_tile():
    run_family(R.family_far_carry())


def test_merge_keeps_tied_starts_in_order_of_production():
    run_family(R.family_tied_starts())


def test_covered_window_keeps_the_sentinel_row():
    from hypad_amd.utils import anomaly_detection_utils as adu
    calls = R.family_covered_random()
    run_family(calls)
    (name, segs, kw), = calls
    # and through the mirror, whose index lookup turns the sentinel's -1 into index[-1] as the reference's does
    index = [np.arange(11, 11 + 3 * len(s), 3) for s in segs]
    got = adu.find_anomalies_signals(torch.from_numpy(np.concatenate(segs)).cuda(), [0] + list(np.cumsum([len(s) for s in segs])),
                                     index_list=index, window_size=kw["window_size"], window_step_size=kw["window_step_size"],
                                     anomaly_padding=kw["anomaly_padding"], min_percent=kw["min_percent"], lower_threshold=kw["lower_threshold"])
    for s, seg in enumerate(segs):
        want = R.host(seg, R.signal_kw(kw, s), index[s])
        assert got[s].shape == want.shape and np.array_equal(got[s][:, :2], want[:, :2]), (s, got[s], want)
        np.testing.assert_allclose(got[s][:, 2], want[:, 2], rtol=R.RTOL, atol=0)
    assert got[0][0, 0] == index[0][-1] and got[0][0, 1] == index[0][-1]
