"""CPU checks of the interval sweep's inputs and allowance (tests/intervals_ref.py), so that tests/test_gpu_intervals_sweep.py may claim
the edges it names: every family has the property that makes it reach its edge (computed with the host helpers _fixed_threshold,
_find_sequences, _get_max_errors, _merge_sequences), every random-valued input meets check_precondition with the score margin, the
derived allowance stays below the contract's rtol 1e-9 on every row of the sweep, and
hypad_find_anomalies_signals_workspace_bytes equals the restatement of fa_windows / fa_layout (the library loads without a GPU)."""
import warnings

import numpy as np
import pytest

import intervals_ref as R
from hypad_amd import _C
from hypad_amd.utils import intervals as iv

BT, LDS_SORT = R.BT, R.LDS_SORT


def _window0(e, kw, s, mirrored=False):
    """(values, threshold, positions above it) of the first window of segment s."""
    w = np.asarray(e[: kw["window_size"][s]], dtype=np.float64)
    if mirrored:
        w = w.mean() - (w - w.mean())
    thr = iv._fixed_threshold(w)
    return w, thr, np.flatnonzero(w > thr)


def _dilated(w, thr, pad):
    return iv._dilate(w > thr, int(pad))


# ------------------------------------------------------------------------------------------------ precondition and allowance
FAMILIES = ("tile_lengths", "tile_offsets", "run_gaps", "sort_runs", "sort_merge", "cap", "degenerate", "mixed", "signs_and_ties", "covered_random",
            "shoulders", "far_carry", "tied_starts")


def test_family_list():
    assert tuple(f for f, _, _ in R.all_calls()) == FAMILIES
    assert tuple(f for f, exact, _ in R.all_calls() if exact) == R.EXACT_FAMILIES


@pytest.mark.parametrize("family", FAMILIES)
def test_every_random_valued_input_meets_the_precondition_and_the_allowance_stays_below_the_contract(family):
    worst, rows = 0.0, 0
    (_, exact, calls), = [c for c in R.all_calls() if c[0] == family]
    for name, segs, kw in calls:
        for s, e in enumerate(segs):
            kw1 = R.signal_kw(kw, s)
            if not exact:
                R.check_precondition(e, kw1, R.MARGIN)
            try:
                table, allowance, merged = R.reference(e, kw1)
            except ZeroDivisionError:
                continue
            if exact:
                allowance, table = allowance[merged], table[merged]          # (unmerged rows of an integer-valued input: bits)
            if len(table):
                assert (allowance > 0).all() and (allowance <= R.RTOL * np.abs(table[:, 2])).all(), (family, name, s)
                worst = max(worst, float((allowance / np.abs(table[:, 2])).max()))
                rows += len(table)
    assert (rows > 0 or exact) and worst < 1e-11                 # (two orders below the contract)


def test_allowance_counts():
    assert R.sum_depth(1) == 16 + 6 + 3 + 1 + 19
    assert R.sum_depth(4096) == 16 + 6 + 3 + 1 + 19 + 5 and R.sum_depth(4097) == 16 + 6 + 3 + 2 + 19 + 6
    assert R.sum_depth(262144) == 16 + 6 + 3 + 64 + 19 + 11
    # the precondition refuses what it is there to refuse
    e = R.spiked(400, [200], 5)
    kw = dict(window_size=400, anomaly_padding=5, min_percent=0.01)       # (at 0.1 the prune would drop a run so close to the rest)
    R.check_precondition(e, kw, R.MARGIN)
    near = e.copy()
    for k in range(60):                                          # (the threshold moves with the value: a contraction)
        near[10] = iv._fixed_threshold(near) * (1 + 1e-9)
    with pytest.raises(AssertionError, match="threshold gap"):
        R.check_precondition(near, kw, R.MARGIN)
    low = e.copy()
    lo, hi = 1.1, 3.5                                            # bisect the spike down to 2 % above its own threshold
    for k in range(60):
        low[200] = 0.5 * (lo + hi)
        lo, hi = (lo, low[200]) if low[200] > 1.02 * iv._fixed_threshold(low) else (low[200], hi)
    low[200] = hi
    assert 0.019 < low[200] / iv._fixed_threshold(low) - 1 < 0.021
    R.check_precondition(low, kw)
    with pytest.raises(AssertionError, match="score margin"):
        R.check_precondition(low, kw, R.MARGIN)


# ------------------------------------------------------------------------------------------------ the families reach their edges
@pytest.mark.parametrize("pad", (63, 0))
def test_tile_lengths_put_values_above_on_every_seam(pad):
    (name, segs, kw), far = R.family_tile_lengths(pad)
    assert R.tile_tail(65, 0) == R.tile_tail(65, 1) == R.tile_tail(65, 64) == R.tile_tail(1023, 63) == 1025 and R.tile_tail(65, 63) == 65
    seen = {}
    for s in range(0, len(segs), 3):
        L, variant = kw["window_size"][s], (s // 3) % 2
        assert len(segs[s]) == L and len(segs[s + 1]) == L + 1 and len(segs[s + 2]) == L + R.tile_tail(L, pad)
        assert segs[s + 2][:L].tobytes() == segs[s].tobytes() and segs[s + 1][:L].tobytes() == segs[s].tobytes()
        w, thr, above = _window0(segs[s], kw, s)
        assert list(above) == R.tile_spikes(L, variant), (L, variant)        # exactly the placed values lie above
        seen.setdefault(L, set()).update(int(p) for p in above)
        # the last, short window of the longest embedding: 1 025 values, one above at its position 512
        tail = segs[s + 2][(len(segs[s + 2]) - 1) // L * L:] if L > 1025 else None
        if tail is not None:
            assert len(tail) == 1025 and list(np.flatnonzero(tail > iv._fixed_threshold(tail))) == [512]
        assert R.fa_windows(L + 1, L, L) == 2 and R.fa_windows(L + R.tile_tail(L, pad), L, L) == -(-R.tile_tail(L, pad) // L) + 1
    assert sorted(seen) == list(R.TILE_LENGTHS)
    for L, pos in seen.items():
        if L < 60:
            assert not pos                                       # (nothing can lie 4 sd above the mean of fewer than 18 values)
            continue
        assert 0 in pos and L - 1 in pos
        for m in range(BT, L, BT):
            assert m - 1 in pos and m in pos, (L, m)
        if L > 65:                                               # both sides of a multiple of 64 that is no multiple of 1 024
            assert any(p % 64 == 63 and p + 1 in pos and (p + 1) % BT for p in pos), L
    assert {-(-L // R.RED_ELEMS) for L in R.TILE_LENGTHS} == {1, 2, 3}
    # the paddings: shorter than a mask word, a word, a tile, longer than a tile, the whole window, beyond int32
    (_, fsegs, fkw) = far
    for s, e in enumerate(fsegs):
        L = len(e)
        w, thr, above = _window0(e, fkw, s)
        assert list(above) == [1000, L - 1000]
        # with padding 1 500 a position two tiles behind 1 000 is still covered from it, and one two tiles in front of L - 1 000
        i = 2 * BT + 100
        assert i // BT - 1000 // BT == 2 and i - 1000 <= 1500 and not (w[BT:i + 1] > thr).any()
        j = (L - 1000) // BT * BT - BT - 100
        assert (L - 1000) // BT - j // BT == 2 and (L - 1000) - j <= 1500 and not (w[j:(L - 1000) // BT * BT] > thr).any()
    for name, segs, kw in R.family_tile_lengths("L"):
        L = kw["anomaly_padding"]
        assert kw["window_size"] == [L] * 6
        for s in (0, 3):
            w, thr, above = _window0(segs[s], kw, s)
            if len(above):                                       # covered entirely by the padded mask: max_below = 0
                assert _dilated(w, thr, L).all() and iv._find_sequences(w, thr, L)[1] == 0
                assert iv._find_sequences(w, thr, L)[0].tolist() == [[0, L - 1]]
    assert [kw["anomaly_padding"] for _, _, kw in R.family_tile_lengths(2 ** 40)] == [2 ** 40] * 2
    for first in R.TILE_OFFSETS:
        (name, segs, kw), = R.family_tile_offsets(first)
        assert len(segs[0]) == first and [len(s) for s in segs[1:]] == [L for L in R.TILE_LENGTHS for _ in (0, 1)]


def test_run_gaps_sit_on_the_tile_seam_and_on_list_entries_1023_and_1024():
    for pad in R.GAP_PADS:
        (name, segs, kw), = R.family_run_gaps(pad)
        ds = R.gap_pairs(pad)
        assert ds == ([1, 2] if pad == 0 else [2 * pad, 2 * pad + 1, 2 * pad + 2]) and len(segs) == 2 * len(ds)
        for k, d in enumerate(ds):
            one_run = d <= 2 * pad + 1
            w, thr, above = _window0(segs[2 * k], kw, 2 * k)
            assert len(above) == 2 and above[1] - above[0] == d and above[0] <= BT - 1 < BT <= above[1]
            assert len(iv._find_sequences(w, thr, pad)[0]) == (1 if one_run else 2)
            w, thr, above = _window0(segs[2 * k + 1], kw, 2 * k + 1)
            assert len(above) > BT + 1 and above[BT - 1] == R.GAP_Q and above[BT] == R.GAP_Q + d
            assert len(above) <= R.fa_layout(len(w), 1, 1)["cap"]
            seqs = iv._find_sequences(w, thr, pad)[0]
            holds = [(a <= R.GAP_Q <= b, a <= R.GAP_Q + d <= b) for a, b in seqs]
            assert ((True, True) in holds) == one_run and ((True, False) in holds) == (not one_run)


def test_sort_families_have_exactly_the_counts_they_name():
    for count in R.SORT_COUNTS:
        (name, segs, kw), = R.family_sort_runs(count)
        w, thr, above = _window0(segs[0], kw, 0)
        assert len(w) == R.SORT_N and len(above) == 2 * count
        seqs, below = iv._find_sequences(w, thr, 0)
        assert len(seqs) == count and (seqs[:, 1] - seqs[:, 0] == 1).all()
        kept = iv._prune_anomalies(iv._get_max_errors(w, seqs, below), 0.1)
        assert len(kept) == count and (kept[:, 0] >= 0).all()     # every run kept, the sentinel behind them
        assert len(R.host(segs[0], R.signal_kw(kw, 0))) == count
    assert R._pow2ceil(4095) == R._pow2ceil(4096) == LDS_SORT < R._pow2ceil(4097)
    for rows in (4096, 4097):
        (name, segs, kw), = R.family_sort_merge(rows)
        kw1 = R.signal_kw(kw, 0)
        assert kw1["window_step_size"] * 4 == kw1["window_size"]
        assert R.handed_rows(segs[0], kw1) == rows
        table = R.host(segs[0], kw1)
        assert len(table) > BT                                   # the scans over the merged groups cross a tile
        assert (table[:, 1] > table[:, 0]).all()


def test_cap_family_is_as_dense_as_the_cap_allows_and_ties_exactly():
    for name, segs, kw in R.family_cap():
        w, thr, above = _window0(segs[0], kw, 0)
        cap = R.fa_layout(len(w), 1, 1)["cap"]
        assert len(w) == 18432 and cap == 1154 and len(above) == 1024 and w.mean() == 1.0 and 17.49 < thr < 17.5
        denser = np.zeros(len(w))
        denser[::17] = 17.0                                      # one value in 17: nothing lies above any more
        assert not (denser > iv._fixed_threshold(denser)).any()
        for e, k in zip(segs[1:], (1, 64, 1025)):
            assert len(e) == 17 * k and (e == 17.0).sum() == k and e.mean() == 1.0 and e.std() == 4.0
            assert iv._fixed_threshold(e) == 17.0 and len(R.host(e, dict(anomaly_padding=kw["anomaly_padding"], lower_threshold=kw["lower_threshold"]))) == 0
    assert {(kw["anomaly_padding"], kw["lower_threshold"]) for _, _, kw in R.family_cap()} == {(0, False), (0, True), (50, False), (50, True)}


def test_degenerate_family_holds_every_degenerate_item():
    for lower in (False, True):
        (name, segs, kw), = R.family_degenerate(lower)
        shapes = [(len(e), a, b) for e, a, b in zip(segs, kw["window_size"], kw["window_step_size"])]
        assert (10, 2, 7) in shapes and R.fa_windows(10, 2, 7) == 3 and 2 * 7 > 10          # the third window starts beyond the segment
        assert (300, 1000, 2000) in shapes and (300, 100, 5000) in shapes and (1, 1, 1) in shapes and (2, 2, 2) in shapes and (1, 5, 3) in shapes
        assert (600, 200, 1) in shapes and R.fa_windows(600, 200, 1) == 401
        for bad in (np.nan, np.inf, -np.inf):
            where = set()
            for e, (n, size, step) in zip(segs, shapes):
                hit = np.flatnonzero(np.isnan(e) if np.isnan(bad) else e == bad)
                if len(hit) == 1 and n == 5000:
                    where.add(int(hit[0]))
                if len(hit) == 1 and n == 12500:
                    assert hit[0] - step == 4096 and hit[0] - 2 * step < size and hit[0] >= size
            assert where == {0, 4096, 4999}
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            tables = [R.host(e, R.signal_kw(kw, s)) for s, e in enumerate(segs)]
        assert sum(len(t) > 0 for t in tables) >= 6 and sum(len(t) == 0 for t in tables) >= 14
        assert all(len(t) > 0 for t, sh in zip(tables, shapes) if sh[0] == 12500)             # their clean windows still report


def test_mixed_family():
    for total in (65, 129):
        (name, segs, kw), = R.family_mixed(total)
        shapes = sorted((len(e), a, b) for e, a, b in zip(segs, kw["window_size"], kw["window_step_size"]))
        assert len(segs) == total and shapes.count((5, 5, 5)) == 5 and (8193, 8193, 8193) in shapes and (600, 200, 1) in shapes
        assert R.fa_layout(8193, 1, 1)["nch"] == 3 and total > R.FA_CHUNK * (total // R.FA_CHUNK)
        lengths = [len(e) for e in segs]
        assert lengths.index(8193) > 0                           # (not at the head of the call)


def test_signs_ties_and_covered_windows():
    calls = R.family_signs_and_ties()
    assert sorted({kw["min_percent"] for _, _, kw in calls}) == [0.0, 0.1, 1.5]
    for name, segs, kw in calls:
        pad, minp = kw["anomaly_padding"], kw["min_percent"]
        if name.startswith("ties"):
            plateaus, mirror, zeros = segs
            w, thr, above = _window0(plateaus, kw, 0)
            seqs, below = iv._find_sequences(w, thr, pad)
            rows = iv._get_max_errors(w, seqs, below)
            assert len(seqs) == 25 and (rows[:-1, 2] == 36.0).all() and (np.diff(rows[:-1, 0]) > 0).all()    # equal maxima, by start
            assert len(iv._prune_anomalies(rows, minp)) == (0 if minp > 1 else 25)
            w, thr, above = _window0(mirror, kw, 1)
            up = iv._get_max_errors(w, *iv._find_sequences(w, thr, pad))
            w2, thr2, above2 = _window0(mirror, kw, 1, mirrored=True)
            down = iv._get_max_errors(w2, *iv._find_sequences(w2, thr2, pad))
            assert thr == thr2 and len(up) == len(down) == 11 and (up[:, 2] == down[:, 2]).all()               # the mirrored window's runs tie
            assert w.mean() == 1.0 and (up[:-1, 0] != down[:-1, 0]).all()
            w, thr, above = _window0(zeros, kw, 2)
            rows = iv._get_max_errors(w, *iv._find_sequences(w, thr, pad))
            assert w.mean() == -17.0 and thr < 0 and len(rows) == 26 and (rows[:-1, 2] == 0.0).all() and rows[-1, 2] == -18.0
            assert len(iv._prune_anomalies(rows, minp)) == 25    # 0 / 0 and 18 / 0 are not below any min_percent
        elif name.startswith("a zero-weight row"):
            rows = [r.tolist() for start, v, pruned, _, _, _ in R.window_rows(segs[0], R.signal_kw(kw, 0)) for r in pruned + [start, start, 0]]
            assert [3599.0, 3599.0, 36.0] in rows and [3599.0, 3602.0, 36.0] in rows
            assert [r[:2] for r in rows].index([3599.0, 3599.0]) < [r[:2] for r in rows].index([3599.0, 3602.0])
            assert [3599.0, 3602.0] in R.host(segs[0], R.signal_kw(kw, 0))[:, :2].tolist()                      # merged, nothing raised
        else:
            for s, e in enumerate(segs[:2]):
                w, thr, above = _window0(e, kw, s)
                assert len(above) == 8 and _dilated(w, thr, pad).all() and w[above].max() == (0.0, -50.0)[s]
                rows = iv._get_max_errors(w, *iv._find_sequences(w, thr, pad))
                assert rows[0, 0] == -1 and rows[0, 2] == 0.0 and len(rows) == 2                                # the sentinel sorts first
                table = R.host(e, R.signal_kw(kw, s))
                assert table[0, :2].tolist() == [len(e) - 1, len(e) - 1] and table[0, 2] == (0.0 - thr) / (w.mean() + w.std())
    (name, segs, kw), = R.family_covered_random()
    w, thr, above = _window0(segs[0], kw, 0)
    assert _dilated(w, thr, 400).all() and w[above].max() < 0
    table = R.host(segs[0], R.signal_kw(kw, 0))
    assert table.shape == (1, 3) and table[0, :2].tolist() == [399.0, 399.0] and -0.9 < table[0, 2] < -0.7
    assert R.host(segs[1], R.signal_kw(kw, 1))[:, 0].tolist() == [799.0, 399.0]      # sorted as -1 and 399: index[-1] of the first window, start - 1 of the second


def test_shoulders_lie_inside_a_run_and_would_prune_everything_outside():
    (name, segs, kw), = R.family_shoulders()
    pad, minp = kw["anomaly_padding"], kw["min_percent"]
    for s, (what, shift, spike, at) in enumerate(R.SHOULDERS):
        w, thr, above = _window0(segs[s], kw, s)
        assert len(w) == R.SHOULDER_L and len(above) == 26 and spike in above and w[at] == R.SHOULDER < thr
        near = above[np.abs(above - at) <= pad]
        assert list(near) == [spike] and _dilated(w, thr, pad)[at]            # covered by that one value above, and by no other
        assert abs(spike - at) == pad or spike // BT != at // BT, what         # on the rim, or across the tile seam
        seqs, below = iv._find_sequences(w, thr, pad)
        rows = iv._get_max_errors(w, seqs, below)
        assert below < 1.11 and len(iv._prune_anomalies(rows, minp)) == 26
        rows[-1, 2] = R.SHOULDER                                             # were it outside: nothing would stand out
        assert len(iv._prune_anomalies(rows, minp)) == 0
    assert {(sp - at > 0, sp // BT != at // BT) for _, _, sp, at in R.SHOULDERS} == {(False, False), (True, False), (False, True), (True, True)}


def test_far_carry_and_tied_starts():
    (name, segs, kw), = R.family_far_carry()
    kw1 = R.signal_kw(kw, 0)
    per_window = [(start, pruned) for start, _, pruned, _, _, _ in R.window_rows(segs[0], kw1)]
    assert [len(p) for _, p in per_window] == [1, R.FAR_PEAKS + 50]
    long = per_window[0][1][0]
    assert (long[0], long[1]) == (R.FAR_AT, R.FAR_AT + 2 * R.FAR_PEAKS - 1)
    rows = sorted(([s + p[0], s + p[1]] for s, pr in per_window for p in pr), key=lambda r: r[0])
    assert rows[0] == [R.FAR_AT, R.FAR_AT + 2 * R.FAR_PEAKS - 1]
    for j in range(BT - 2, BT + 3):                                         # around sorted row 1 024: zero-length rows two apart, inside the first row
        assert rows[j][0] == rows[j][1] == rows[j - 1][1] + 2 < rows[0][1]
    table = R.host(segs[0], kw1)
    assert len(table) == 51 and table[0, :2].tolist() == rows[0]
    (name, segs, kw), = R.family_tied_starts()
    at = float(R.TIED_AT)
    for s, early in enumerate(R.TIED_EARLY):
        kw1 = R.signal_kw(kw, s)
        rows = [[a + p[0], a + p[1]] for a, _, pr, _, _, _ in R.window_rows(segs[s], kw1) for p in pr]
        tied = [r for r in rows if r[0] == at]                   # in order of production: weights 0, 1, then 0 throughout
        assert tied[:2] == [[at, at], [at, at + 1]] and tied[2:] == [[at, at]] * 398 and rows.count([at + 2, at + 2]) == 400
        assert rows.index([at, at]) == sum(r[0] < at for r in rows) and (len(rows) > 800) == bool(early)
        assert R.host(segs[s], kw1)[:, :2].tolist() == [[float(p), p + 1.0] for p in early] + [[at, at + 2]]


# ------------------------------------------------------------------------------------------------ the workspace
def _bytes(lengths, sizes, steps, lower):
    off = [0] + [int(v) for v in np.cumsum(lengths)]
    return _C.lib.hypad_find_anomalies_signals_workspace_bytes(len(lengths), _C.int64s(off), _C.int64s(sizes), _C.int64s(steps), int(lower))


def test_workspace_bytes_equal_the_restated_layout():
    assert R.fa_windows(10, 2, 7) == 3 and R.fa_windows(10, 10, 1) == 1 and R.fa_windows(11, 10, 1) == 2 and R.fa_windows(600, 200, 1) == 401
    for n in range(1, 71):
        combos = [(size, step) for size in range(1, n + 3) for step in range(1, n + 3)]
        for lower in (0, 1):
            want = R.workspace_bytes([n] * len(combos), [c[0] for c in combos], [c[1] for c in combos], lower)
            assert _bytes([n] * len(combos), [c[0] for c in combos], [c[1] for c in combos], lower) == want, (n, lower)
        if n <= 12 or n in (64, 65, 70):                         # and one signal at a time, so that no two errors can cancel
            for size, step in combos:
                for lower in (0, 1):
                    assert _bytes([n], [size], [step], lower) == R.workspace_bytes([n], [size], [step], lower), (n, size, step, lower)
    # where cap = size / 16 + 2 and its power of two move
    for size in (16367, 16368, 16369, 65519, 65520, 65521, 65535, 65536, 65537):
        lay = R.fa_layout(size, 1, 1)
        assert lay["cap"] == size // 16 + 2 and lay["P"] >= lay["cap"] > lay["P"] // 2
        for n, step in ((size, size), (size + 1, size), (2 * size + 3, size // 3), (size - 1, 5)):
            for lower in (0, 1):
                assert _bytes([n], [size], [step], lower) == R.workspace_bytes([n], [size], [step], lower), (size, n, step, lower)
    assert R.fa_layout(16367, 1, 1)["P"] == 1024 < R.fa_layout(16368, 1, 1)["P"] == 2048
    assert R.fa_layout(65519, 1, 1)["P"] == 4096 < R.fa_layout(65520, 1, 1)["P"] == R.fa_layout(65536, 1, 1)["P"] == 8192
    # every call of the sweep
    for family, exact, calls in R.all_calls():
        for name, segs, kw in calls:
            lengths = [len(e) for e in segs]
            assert _bytes(lengths, kw["window_size"], kw["window_step_size"], kw["lower_threshold"]) == \
                R.workspace_bytes(lengths, kw["window_size"], kw["window_step_size"], kw["lower_threshold"]) > 0, (family, name)
