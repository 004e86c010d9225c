"""Reference, allowance and inputs of the interval-extraction sweep (tests/test_gpu_intervals_sweep.py on the GPU,
tests/test_intervals_reference.py on the CPU; tests/test_gpu_find_anomalies_signals.py takes its helpers from here).

The reference is ``hypad_amd.utils.intervals.find_anomalies(..., fixed_threshold=True)`` in fp64 NumPy, which tests/golden/intervals.npz
pins to the original project's outputs.  Nothing here models the kernel's order of operations: ``reference`` calls the host function
for the table and walks the same windows with the host helpers only to attach an allowance to every row.

``fa_windows`` / ``fa_layout`` restate the workspace arithmetic of csrc/intervals.hip from its comments, for the ctypes check of
``hypad_find_anomalies_signals_workspace_bytes``.

The families return lists of ``(name, segments, kwargs)``: the segments of one C call and its arguments, ``window_size`` and
``window_step_size`` one value per segment.  Random-valued families are seeded until every segment meets ``check_precondition``;
that happens here, on the CPU, never by filtering at run time.
"""
import functools
import math
import warnings

import numpy as np

RTOL = 1e-9                 # the contract of find_anomalies_signals; the derived allowance must stay below it
GAP = 1e-6
MARGIN = 0.05
U = 2.0 ** -53
BT, RED_T, RED_ELEMS, LDS_SORT, FA_CHUNK = 1024, 256, 4096, 4096, 64      # the constants of csrc/intervals.hip


# ------------------------------------------------------------------------------------------------ moved from the GPU test
def series(n, spikes, width, seed, plateau=False):
    """Noise plus spikes, as tests/golden/gen_fixtures.py makes the interval fixtures."""
    r = np.random.default_rng(seed)
    e = 1.0 + 0.1 * np.abs(r.standard_normal(n))
    for k in range(spikes):
        c = int(r.integers(0, n))
        w = int(r.integers(1, width + 1))
        e[c: c + w] += r.uniform(0.8, 3.0) if not plateau else 2.0
    return e


def _sizes(n, kw):
    size = kw.get("window_size") or n
    if kw.get("window_size_portion"):
        size = int(np.ceil(n * kw["window_size_portion"]))
    step = kw.get("window_step_size") or size
    if kw.get("window_step_size_portion"):
        step = int(np.ceil(size * kw["window_step_size_portion"]))
    return size, step


def _windows(e, kw):
    size, step = _sizes(e.size, kw)
    start = end = 0
    while end < e.size:
        end = start + size
        w = e[start:end]
        yield w
        if kw.get("lower_threshold"):
            yield w.mean() - (w - w.mean())
        start += step


def check_precondition(e, kw, margin=0.0):
    """No value within GAP (relative) of its window's threshold, no prune ratio within GAP of min_percent, and (the sweep asks
    ``margin=MARGIN``) every kept run's maximum above its window's threshold by at least ``margin`` of the threshold, so that the score
    (max - thr) / (mean + sd) is no cancellation.  A window with a NaN or an infinity has no threshold (nothing to be near to), an empty
    one (a step beyond the segment) neither; an exactly constant window of an integer value sums exactly in any order, so its mean is
    that value and its standard deviation 0 on both sides -- nothing lies above the threshold, which equals the value."""
    from hypad_amd.utils import intervals as iv
    e = np.asarray(e, dtype=np.float64)
    minp, pad = kw.get("min_percent", 0.1), kw.get("anomaly_padding", 50)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for w in _windows(e, kw):
            if w.size <= 1 or not np.isfinite(w).all():       # (one value: its own mean, sd 0, on both sides)
                continue
            if (w == w[0]).all():
                assert w[0] == np.round(w[0]) and abs(w[0]) * w.size < 2.0 ** 53
                continue
            thr = iv._fixed_threshold(w)
            assert np.abs(w - thr).min() > GAP * abs(thr), ("threshold gap", np.abs(w - thr).min() / abs(thr))
            seqs, below = iv._find_sequences(w, thr, pad)
            rows = iv._get_max_errors(w, seqs, below)
            me = rows[:, 2]
            if me.size > 1:
                ratio = (me[:-1] - me[1:]) / me[:-1]
                assert np.abs(ratio - minp).min() > GAP, ("prune gap", np.abs(ratio - minp).min())
            if margin:
                for s, _, mx in iv._prune_anomalies(rows, minp):
                    if s >= 0:                               # (the sentinel's own row scores (0 - thr): exact numerator)
                        assert mx - thr >= margin * abs(thr), ("score margin", (mx - thr) / abs(thr))


def host(e, kw, index=None):
    from hypad_amd.utils import intervals as iv
    index = np.arange(e.size) if index is None else index
    with np.errstate(all="ignore"), warnings.catch_warnings():     # (an empty or a non-finite window: NumPy warns, the result stands)
        warnings.simplefilter("ignore")
        return np.asarray(iv.find_anomalies(e, index, **dict(kw, fixed_threshold=True)), dtype=np.float64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ the score allowance
# First order in U = 2^-53.  Both sides compute the same expressions from the same values and differ only in the order of the two
# sums of a window (and, for a merged row, of the weighted average).
#
# * A sum of L terms.  The kernel adds at most RED_ELEMS / RED_T = 16 values per thread, then 6 butterfly steps, 3 additions for the
#   four wave sums, then the ceil(L / 4096) chunk sums in order: a term passes through at most k_dev = 16 + 6 + 3 + nch additions.
#   NumPy sums pairwise: blocks of at most 128 values in 8 interleaved accumulators (16 additions, 3 to combine them), and one more
#   addition per halving above that: k_np = 19 + ceil(log2(L / 128)).  Each side is within k U sum|t| of the exact sum, so the two are
#   within K U sum|t| of one another, K = k_dev + k_np.
# * mean = sum x / L.  With one division on either side: |d mean| <= e_m = (K + 2) U mean|x|.
# * v = sum (x - mean)^2 / L.  A shift of the mean by d changes sum (x - mean)^2 by -2 d sum (x - mean) + L d^2; sum (x - mean) is itself
#   of the order L e_m, so that is second order.  A deviation is rounded once (U |dev|), entering the square twice, the square once,
#   then the sum (all terms positive: relative) and the division: (3 + k + 1) U relative on either side, (K + 8) U between the two.
#   sd = sqrt(v): half of that plus one rounding on either side, e_sd = sd ((K + 8) / 2 + 2) U.
# * thr = mean + 4 sd (4 sd is exact) and denom = mean + sd, one rounded addition on either side:
#   d_thr = e_m + 4 e_sd + 2 U |thr|,  d_den = e_m + e_sd + 2 U |denom|.
# * The mirrored window of lower_threshold, x' = mean - (x - mean), is formed on either side from its own mean: every element moves by
#   the common shift 2 e_m and, through the two roundings, by at most 2 U (|x - mean| + |x'|) more.  The shift adds to the mean's
#   error and cancels in the deviations; the roundings add 2 U (mean|x - mean| + mean|x'|) to e_m and, through 2 sum dev' r / L with
#   sum |dev'| |x'| <= L sd rms(x'), 4 U (1 + rms(x') / sd) to the relative error of v.  A maximum of the mirrored window carries the
#   same shift and roundings; a maximum of the window itself is an input value, equal on both sides.
# * score = (max - thr) / denom, one subtraction and one division on either side:
#   a = (d_max + d_thr + 2 U |max - thr|) / |denom| + |score| d_den / |denom| + 2 U |score|.
#   check_precondition(margin=MARGIN) keeps max - thr >= 0.05 |thr|, so a / |score| stays a small multiple of K U.
# * A merged row is np.average(scores, weights = stop - start) over its n rows; the weights are integers, exact.  The errors of the
#   rows pass through with their weights, and the n products, the two sums (sequential in the kernel, pairwise in NumPy, n - 1
#   additions at the most on either side) and the division add at most (2 n + 4) U sum w |s| / sum w.  n is bounded by the number of
#   rows the signal's windows produce in all.
def sum_depth(L):
    k_dev = RED_ELEMS // RED_T + 6 + 3 + -(-L // RED_ELEMS)
    k_np = 19 + max(0, math.ceil(math.log2(max(L, 1) / 128.0)))
    return k_dev + k_np


def stats_allowance(w, shift=0.0, mirrored=False):
    """(e_m, d_thr, d_den) of one window as the host sees it; ``shift``: the common shift of its elements between the two sides."""
    K = sum_depth(w.size)
    mean, sd = w.mean(), w.std()
    mabs = np.abs(w).mean()
    e_m = (K + 2) * U * mabs + shift
    rel_v = (K + 8) * U
    if mirrored:
        e_m += 2 * U * (np.abs(w - mean).mean() + mabs)
        rel_v += 4 * U * (1.0 + (math.sqrt((w * w).mean()) / sd if sd > 0 else 0.0))
    e_sd = sd * (rel_v / 2 + 2 * U)
    return e_m, e_m + 4 * e_sd + 2 * U * abs(mean + 4 * sd), e_m + e_sd + 2 * U * abs(mean + sd)


def window_rows(e, kw):
    """Per (window, pass) in the order find_anomalies visits them: (window_start, values, pruned rows of _get_max_errors,
    threshold, shift of the values between the two sides, mirrored).  Host helpers only."""
    from hypad_amd.utils import intervals as iv
    e = np.asarray(e, dtype=np.float64)
    minp, pad = kw.get("min_percent", 0.1), kw.get("anomaly_padding", 50)
    size, step = _sizes(e.size, kw)
    start = end = 0
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        while end < e.size:
            end = start + size
            w = e[start:end]
            passes = [(w, 0.0, False)]
            if kw.get("lower_threshold"):
                passes.append((w.mean() - (w - w.mean()), 2 * stats_allowance(w)[0] if w.size else 0.0, True))
            for v, shift, mirrored in passes:
                if v.size == 0 or not np.isfinite(v).all():
                    yield start, v, np.zeros((0, 3)), np.nan, shift, mirrored
                    continue
                thr = iv._fixed_threshold(v)
                seqs, below = iv._find_sequences(v, thr, pad)
                yield start, v, iv._prune_anomalies(iv._get_max_errors(v, seqs, below), minp), thr, shift, mirrored
            start += step


def reference(e, kw):
    """(table, allowance, merged): ``host(e, kw)``, per row the bound on |device score - host score| derived above, and whether the row
    is an average of several.  Raises ZeroDivisionError where the host does."""
    from hypad_amd.utils import intervals as iv
    e = np.asarray(e, dtype=np.float64)
    table = host(e, kw)
    rows_a, rows_s = [], []
    for start, v, pruned, thr, shift, mirrored in window_rows(e, kw):
        if not len(pruned):
            continue
        _, d_thr, d_den = stats_allowance(v, shift, mirrored)
        mean = v.mean()
        den = mean + v.std()
        for s, t, mx in pruned:
            d_max = shift + 2 * U * (abs(mx - mean) + abs(mx)) if mirrored and s >= 0 else 0.0
            sc = (mx - thr) / den
            a = (d_max + d_thr + 2 * U * abs(mx - thr)) / abs(den) + abs(sc) * d_den / abs(den) + 2 * U * abs(sc)
            rows_a.append([s + start, t + start, a])
            rows_s.append([s + start, t + start, abs(sc)])
    if not rows_a:
        assert table.shape == (0, 3)
        return table, np.zeros(0), np.zeros(0, dtype=bool)
    ma, ms = iv._merge_sequences(rows_a), iv._merge_sequences(rows_s)
    assert np.array_equal(np.arange(e.size)[ma[:, :2].astype(np.int64)], table[:, :2])
    starts = np.sort(np.asarray(rows_a)[:, 0])
    members = np.searchsorted(starts, ma[:, 1], side="right") - np.searchsorted(starts, ma[:, 0], side="left")
    merged = members > 1
    allowance = ma[:, 2] + np.where(merged, (2 * len(rows_a) + 4) * U * ms[:, 2], 0.0)
    return table, allowance, merged


# ------------------------------------------------------------------------------------------------ the workspace, restated
def fa_windows(n, size, step):
    """Windows of a segment of n values: the `while window_end < n` of find_anomalies."""
    return (n - size + step - 1) // step + 1 if n > size else 1


def _pow2ceil(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def _up8(b):
    return (b + 7) & ~7


def fa_layout(size, nw, passes):
    """Workspace of one signal, from the comment of FaLayout: [4 partial sums per (window, chunk) | kept count per item | its offset in
    the candidate list | item blocks | the candidate list and its sort].  An item block: value and key per value above the threshold
    (cap of them), the sort's 64-bit keys (P), the left-cover mask words, position / run number / run start / run end (32-bit, cap
    each), the sort's 32-bit payload (P), rounded up to 8 bytes."""
    cap = size // 16 + 2
    P = _pow2ceil(cap)
    nch = -(-size // RED_ELEMS)
    words = -(-size // BT) * (BT // 64)
    NI = nw * passes
    gcap = NI * cap
    Pg = _pow2ceil(gcap)
    IB = _up8(cap * 8 + cap * 8 + P * 8 + words * 8 + 4 * cap * 4 + P * 4)
    o = nw * nch * 4 * 8 + 2 * _up8(NI * 4) + NI * IB
    o += gcap * 8 + Pg * 8 + 3 * _up8(gcap * 4) + _up8(Pg * 4)
    return dict(cap=cap, P=P, nch=nch, words=words, NI=NI, gcap=gcap, Pg=Pg, IB=IB, bytes=(o + 255) & ~255)


def workspace_bytes(lengths, sizes, steps, lower):
    total = 0
    for n, size, step in zip(lengths, sizes, steps):
        size, step = min(size, n), min(step, n)
        total += fa_layout(size, fa_windows(n, size, step), 2 if lower else 1)["bytes"]
    return total


# ------------------------------------------------------------------------------------------------ the inputs of the sweep
def signal_kw(kw, s):
    """The arguments of find_anomalies for segment s of a call."""
    return dict(kw, window_size=kw["window_size"][s], window_step_size=kw["window_step_size"][s])


def spiked(n, positions, seed, width=1, lo=2.0, hi=2.5, normal=False):
    """Noise with `width` points raised by a height in lo .. hi at every position.  The noise is 1 + 0.1 U(0, 1), which never reaches
    mean + 4 sd on its own (a uniform variable ends 1.73 sd above its mean), so that the values above a threshold are the spikes
    placed here and nothing else; ``normal``: 1 + 0.1 |N(0, 1)|, for windows whose spikes lift the threshold far out of its reach."""
    r = np.random.default_rng(seed)
    e = 1.0 + 0.1 * (np.abs(r.standard_normal(n)) if normal else r.uniform(size=n))
    for p in positions:
        k = min(width, n - p)
        e[p: p + k] += r.uniform(lo, hi, size=k)
    return e


def _call(segs, pad=50, minp=0.1, lower=False, sizes=None, steps=None):
    sizes = [len(s) for s in segs] if sizes is None else list(sizes)
    steps = list(sizes) if steps is None else list(steps)
    return [np.ascontiguousarray(s, dtype=np.float64) for s in segs], dict(window_size=sizes, window_step_size=steps, anomaly_padding=pad,
                                                                              min_percent=minp, lower_threshold=lower)


def pick(make, seed, size=None, step=None, pad=50, lower=False, minp=0.1, tries=200):
    """make(seed) for the first seed from `seed` on (in steps of 1 000) whose series meets check_precondition(margin=MARGIN)."""
    for k in range(tries):
        e = np.ascontiguousarray(make(seed + 1000 * k), dtype=np.float64)
        kw = dict(window_size=len(e) if size is None else size, window_step_size=step, anomaly_padding=pad, min_percent=minp,
                  lower_threshold=lower)
        try:
            check_precondition(e, kw, MARGIN)
        except AssertionError:
            continue
        return e
    raise AssertionError("no seed meets the precondition")


# 1. tile and chunk lengths
TILE_LENGTHS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 8192, 8193)
TILE_PADS = (0, 1, 63, 64, 1023, 1024, 1500, "L", 2 ** 31 + 5, 2 ** 40)
TILE_OFFSETS = (1, 3, 1025)
TILE_FAR = (4095, 4096, 4097, 8192, 8193)


def tile_spikes(L, variant):
    """Variant 0: the position below every multiple of 1 024, position 0, the position below one multiple of 64.  Variant 1: every
    multiple of 1 024, L - 1, that multiple of 64.  At most L // 30 of them, so that every one stays well above mean + 4 sd.
    Variant 2: positions 1 000 and L - 1 000, so that the forward carry of the last value above and the backward carry of the next one
    pass through tiles that hold none."""
    ms = list(range(BT, L, BT))
    m64 = 64 * max(1, (L // 2) // 64)
    if m64 % BT == 0:
        m64 += 64
    if variant == 0:
        want = [m - 1 for m in ms] + [0] + ([m64 - 1] if m64 < L else [])
    elif variant == 1:
        want = ms + [L - 1] + ([m64] if m64 < L else [])
    else:                                                        # variant 2 (L >= 4 095): two values with whole tiles between them
        want = [1000, L - 1000]
    return sorted(set(p for p in want[: L // 30] if 0 <= p < L))


TILE_LONG_TAIL_PADS = (0, 1, 64)


def tile_tail(L, pad):
    """Values behind the window in the longest embedding: 1 025.  For the lengths below a tile that is up to 1 026 windows on the host,
    so they have it at three paddings (none, one smaller and one larger than the short windows) and 65 values, a few windows, at the
    others."""
    return 1025 if L >= BT - 1 or pad in TILE_LONG_TAIL_PADS else 65


def _tile_segments(lengths, pad, seed, variants=(0, 1), embedded=True):
    """Per length and variant: the window alone, as the first window of a signal one value longer (a last window of 1), and of a
    signal 1 025 values longer (a last window that crosses a tile, with one spike of its own in its middle; see tile_tail)."""
    segs, sizes = [], []
    for L in lengths:
        for variant in variants:
            p = L if pad == "L" else pad
            tail = tile_tail(L, pad)
            long = pick(lambda sd: spiked(L + tail, tile_spikes(L, variant) + [L + tail // 2], sd), seed + 7 * L + variant, size=L, step=L, pad=p)
            for extra in ((0, 1, tail) if embedded else (0,)):
                segs.append(long[: L + extra])
                sizes.append(L)
    return segs, sizes


@functools.lru_cache(maxsize=None)
def family_tile_lengths(pad):
    """One call per padding (per length for the padding "L", the window's own length)."""
    calls = []
    for lengths in ([TILE_LENGTHS] if pad != "L" else [(L,) for L in TILE_LENGTHS]):
        segs, sizes = _tile_segments(lengths, pad, 100)
        calls.append((f"pad {pad} L {lengths[0] if pad == 'L' else 'all'}",) + _call(segs, pad=lengths[0] if pad == "L" else pad, sizes=sizes))
    if pad != "L":
        segs, sizes = _tile_segments(TILE_FAR, pad, 200, variants=(2,), embedded=False)
        calls.append((f"pad {pad} two far values",) + _call(segs, pad=pad, sizes=sizes))
    return calls


@functools.lru_cache(maxsize=None)
def family_tile_offsets(first):
    """The windows of family 1 (alone) behind a first segment of `first` doubles."""
    segs, sizes = _tile_segments(TILE_LENGTHS, 63, 300)
    return [(f"offset {first}",) + _call([spiked(first, [], 301)] + segs[::3], pad=63, sizes=[first] + sizes[::3])]


# 2. run-gap edges
GAP_PADS = (0, 1, 50, 600)
GAP_L1, GAP_L2, GAP_Q = 4096, 65536, 8 + 4 * 1023


def gap_pairs(pad):
    return [d for d in (2 * pad, 2 * pad + 1, 2 * pad + 2) if d > 0]


def gap_positions(d, placement):
    """placement 0: two values above, d apart, on either side of position 1 024.  placement 1: 1 023 values above four positions apart,
    then list entries 1 023 (at GAP_Q) and 1 024 (at GAP_Q + d), then 40 more far behind."""
    if placement == 0:
        p1 = BT - max(1, d // 2)
        return [p1, p1 + d]
    return [8 + 4 * j for j in range(1023)] + [GAP_Q, GAP_Q + d] + [GAP_Q + d + 5000 + 7 * i for i in range(40)]


@functools.lru_cache(maxsize=None)
def family_run_gaps(pad):
    segs = []
    for d in gap_pairs(pad):
        segs.append(pick(lambda sd: spiked(GAP_L1, gap_positions(d, 0), sd), 500 + d, pad=pad))
        segs.append(pick(lambda sd: spiked(GAP_L2, gap_positions(d, 1), sd, lo=2.5, hi=3.0), 501 + d, pad=pad))
    return [(f"pad {pad}",) + _call(segs, pad=pad)]


# 3. both sides of the LDS sort
SORT_N = 262144
SORT_COUNTS = (4095, 4096, 4097)


@functools.lru_cache(maxsize=None)
def family_sort_runs(count):
    """One window of 262 144 values (1 + 0.1 |N(0, 1)| noise) with `count` two-point spikes, padding 0: that many runs, all kept."""
    e = pick(lambda sd: spiked(SORT_N, [30 + 60 * i for i in range(count)], sd, width=2, normal=True), count, pad=0)
    return [(f"{count} runs",) + _call([e], pad=0)]


MERGE_SIZE, MERGE_STEP, MERGE_N = 8192, 2048, 8192 + 2048 * 64


def handed_rows(e, kw):
    """Rows the windows of a signal hand to the merge."""
    return sum(len(pruned) for _, _, pruned, _, _, _ in window_rows(e, kw))


@functools.lru_cache(maxsize=None)
def family_sort_merge(rows):
    """Overlapping windows (step = size / 4), two-point spikes 128 apart from position 2 048 on (four rows each where four windows
    see them) and as many more inside the first step, which only the first window sees (one row each), as make the windows hand the
    merge exactly `rows` rows."""
    kw1 = dict(window_size=MERGE_SIZE, window_step_size=MERGE_STEP, anomaly_padding=0, min_percent=0.1)
    base = [MERGE_STEP + 64 + 128 * i for i in range((MERGE_N - MERGE_STEP) // 128 - 1)]

    def make(seed):
        lo, hi = 0, len(base)
        while lo < hi:                                           # the most spikes that hand over at most `rows` rows
            mid = (lo + hi + 1) // 2
            if handed_rows(spiked(MERGE_N, base[:mid], seed, width=2), kw1) <= rows:
                lo = mid
            else:
                hi = mid - 1
        for extra in range(0, 40):
            e = spiked(MERGE_N, [40 + 48 * i for i in range(extra)] + base[:lo], seed, width=2)
            if handed_rows(e, kw1) == rows:
                return e
        raise AssertionError("row count not reached")
    e = pick(make, 40 + rows, size=MERGE_SIZE, step=MERGE_STEP, pad=0)
    return [(f"{rows} rows",) + _call([e], pad=0, sizes=[MERGE_SIZE], steps=[MERGE_STEP])]


# 4. the cap (integer values: every sum is exact in any order)
def family_cap():
    dense = np.zeros(18432)
    dense[17::18] = 18.0
    calls = []
    for pad in (0, 50):
        for lower in (False, True):
            segs = [dense]
            for k in (1, 64, 1025):
                tie = np.zeros(17 * k)
                tie[8::17] = 17.0
                segs.append(tie)
            calls.append((f"pad {pad} lower {lower}",) + _call(segs, pad=pad, lower=lower))
    return calls


# 5. empty and degenerate items
@functools.lru_cache(maxsize=None)
def family_degenerate(lower):
    segs, sizes, steps = [], [], []

    def add(make, seed, size=None, step=None):
        e = pick(make, seed, size=size, step=step, pad=50, lower=lower)
        segs.append(e)
        sizes.append(len(e) if size is None else size)
        steps.append(sizes[-1] if step is None else step)
    add(lambda sd: spiked(1500, [700], sd), 700, 500, 150)                                     # ordinary
    add(lambda sd: spiked(10, [], sd), 701, 2, 7)                                              # the third window starts beyond the segment
    add(lambda sd: spiked(300, [150], sd), 702, 1000, 2000)                                    # size and step larger than n
    add(lambda sd: spiked(300, [100], sd), 703, 100, 5000)                                     # step larger than n
    add(lambda sd: spiked(600, [100, 300, 480], sd, width=3), 704, 200, 1)                     # 401 windows
    add(lambda sd: spiked(1, [], sd), 705)
    add(lambda sd: spiked(2, [], sd), 706)
    add(lambda sd: spiked(1, [], sd), 707, 5, 3)

    def broken(n, positions, where, bad, width=1):
        def make(sd):
            e = spiked(n, positions, sd, width=width)
            e[where] = bad
            return e
        return make
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for where in (0, 4999, 4096):                                                          # one window of 5 000
            add(broken(5000, [2500], where, bad), 710 + k)
        # windows of 5 000 every 2 500: position 4 096 of window 1, 1 596 of window 2; windows 0 and 3 are clean
        add(broken(12500, [1000, 11000], 2500 + 4096, bad, width=3), 720 + k, 5000, 2500)
    add(lambda sd: spiked(1500, [300, 900], sd, width=4), 730, 500, 150)                       # ordinary
    return [(f"lower {lower}",) + _call(segs, pad=50, lower=lower, sizes=sizes, steps=steps)]


# 6. mixed group
def _ordinary(n, seed):
    r = np.random.default_rng(seed)
    return spiked(n, sorted(int(p) for p in r.integers(0, n - 12, size=2 + seed % 4)), seed, width=1 + seed % 9, lo=1.0, hi=3.0)


@functools.lru_cache(maxsize=None)
def family_mixed(total):
    """One signal with an 8 193-point window (3 reduction chunks), five signals of 5 points, one signal with 401 windows, and ordinary
    signals (windows of a third, steps of a tenth of that) up to `total` signals, in a fixed shuffled order."""
    segs = [pick(lambda sd: spiked(8193, tile_spikes(8193, 0), sd), 900)] + [spiked(5, [], 901 + k) for k in range(5)]
    sizes, steps = [8193] + [5] * 5, [8193] + [5] * 5
    segs.append(pick(lambda sd: spiked(600, [100, 300, 480], sd, width=3), 906, size=200, step=1))
    sizes.append(200)
    steps.append(1)
    k = 0
    while len(segs) < total:
        n = 700 + 13 * k
        sizes.append(int(np.ceil(n * 0.33)))
        steps.append(int(np.ceil(sizes[-1] * 0.1)))
        segs.append(pick(lambda sd: _ordinary(n, sd), 910 + k, size=sizes[-1], step=steps[-1]))
        k += 1
    order = np.random.default_rng(total).permutation(len(segs))
    return [(f"{total} signals",) + _call([segs[i] for i in order], pad=50, sizes=[sizes[i] for i in order], steps=[steps[i] for i in order])]


# 7. signs and ties (integer values but for the one random covered window)
def _plateaus():
    e = np.zeros(3600)                                           # 25 plateaus of four points at 36: mean 1, variance 35
    for k in range(25):
        e[100 + 140 * k: 104 + 140 * k] = 36.0
    return e


def _mirror_ties():
    e = np.ones(3600)                                            # mean 1; 36 above and -34 below mirror into one another
    for k in range(10):
        e[200 + 300 * k: 205 + 300 * k] = 36.0
        e[205 + 300 * k + (k % 2) * 100: 210 + 300 * k + (k % 2) * 100] = -34.0     # touching the plateau above, or 100 behind it
    return e


def _zero_maxima():
    e = np.full(1800, -18.0)                                     # mean -17, variance 17: threshold -0.51, every run maximum is 0
    for k in range(25):
        e[50 + 70 * k: 54 + 70 * k] = 0.0
    return e


def _cut_spike():
    """Windows of 3 600 every 1 800, each with 100 values of 36 (mean 1, variance 35).  The four values from 3 599 on are one point at the
    end of the first window and a run of four in the second: with padding 0 the rows (3 599, 3 599) and (3 599, 3 602) merge, the
    zero-weight one first, and np.average has nothing to complain about."""
    e = np.zeros(5400)
    for k in range(12):
        e[100 + 140 * k: 104 + 140 * k] = 36.0
        e[1900 + 140 * k: 1904 + 140 * k] = 36.0
        e[3700 + 140 * k: 3704 + 140 * k] = 36.0
    e[1750:1753] = 36.0
    e[3599:3603] = 36.0
    return e


def covered_exact(value):
    e = np.full(400, -100.0)                                     # value 0: mean -98, sd 14; value -50: mean -99, sd 7
    e[40:360:40] = value
    return e


def covered_random(seed=0, n=400):
    r = np.random.default_rng(seed)
    e = -10.0 - 0.1 * np.abs(r.standard_normal(n))
    e[100:103] = -5.0
    e[300] = -4.0
    return e


def family_signs_and_ties():
    calls = []
    for minp in (0.0, 0.1, 1.5):
        for lower in (False, True):
            calls.append((f"ties min_percent {minp} lower {lower}",) + _call([_plateaus(), _mirror_ties(), _zero_maxima()], pad=3, minp=minp, lower=lower))
    calls.append(("a zero-weight row in front of its group",) + _call([_cut_spike(), _plateaus()], pad=0, sizes=[3600, 3600], steps=[1800, 3600]))
    for lower in (False, True):
        two = np.concatenate([covered_exact(-50.0), covered_exact(0.0)])
        segs = [covered_exact(0.0), covered_exact(-50.0), two, -covered_exact(-50.0), two]
        calls.append((f"covered exact lower {lower}",) + _call(segs, pad=400, lower=lower, sizes=[400, 400, 400, 400, 800]))
    return calls


@functools.lru_cache(maxsize=None)
def family_covered_random():
    """The covered window with negative run maxima on random values: alone, as the second window of a signal, beside an ordinary one."""
    a = pick(covered_random, 0, pad=400)
    b = pick(covered_random, 1, pad=400)
    return [("covered random",) + _call([a, np.concatenate([b, a]), pick(lambda sd: spiked(400, [200], sd), 2, pad=400)], pad=400, sizes=[400, 400, 400])]


# 8. what the mutation check asked for: inputs on which the padded mask, its carries and the merge's orders decide a result
SHOULDER, SHOULDER_L, SHOULDER_PAD, SHOULDER_MINP = 2.2, 1100, 10, 0.3
SHOULDERS = (("right rim", 0, 500, 510), ("left rim", 0, 500, 490), ("behind the tile seam", 0, 1020, 1026), ("in front of the tile seam", 10, 1030, 1022))


def _shoulder(shift, at, seed):
    e = spiked(SHOULDER_L, [20 + shift + 40 * i for i in range(26)], seed, lo=1.9, hi=1.95)
    e[at] = SHOULDER
    return e


@functools.lru_cache(maxsize=None)
def family_shoulders():
    """26 runs (padding 10) of maxima 2.9 .. 3.05 and one value of 2.2, below the threshold and inside one run's padding: on its rim, or
    across the tile seam from the value above.  Inside, it does not count for max_below (about 1.1) and every run is kept at
    min_percent 0.3; counted as outside, (2.9 - 2.2) / 2.9 < 0.3 would prune them all."""
    segs = [pick(lambda sd: _shoulder(shift, at, sd), 1100 + k, pad=SHOULDER_PAD, minp=SHOULDER_MINP) for k, (_, shift, _, at) in enumerate(SHOULDERS)]
    return [("shoulders",) + _call(segs, pad=SHOULDER_PAD, minp=SHOULDER_MINP)]


FAR_SIZE, FAR_STEP, FAR_AT, FAR_PEAKS = 65536, 32768, 40000, 1050


def _far_carry(seed):
    r = np.random.default_rng(seed)
    e = 1.0 + 0.1 * r.uniform(size=FAR_SIZE + FAR_STEP)
    e[FAR_AT: FAR_AT + 2 * FAR_PEAKS] += 2.2                                     # the first window: one run of 2 100 values
    e[FAR_AT + 1: FAR_AT + 2 * FAR_PEAKS: 2] += r.uniform(0.8, 0.85, size=FAR_PEAKS)     # the second: its threshold lies above the plateau
    for k in range(50):
        e[70000 + 100 * k: 70002 + 100 * k] += r.uniform(9.0, 9.5, size=2)
    return e


@functools.lru_cache(maxsize=None)
def family_far_carry():
    """Two windows, padding 0.  The first reports one row of 2 100 values; the second, whose threshold 50 large spikes lift above that
    plateau, every other value of it as a row of its own: 1 050 zero-length rows inside the first row's span, so that from sorted row
    1 024 on only the carried largest stop joins them to it."""
    e = pick(_far_carry, 1200, size=FAR_SIZE, step=FAR_STEP, pad=0)
    return [("far carry",) + _call([e], pad=0, sizes=[FAR_SIZE], steps=[FAR_STEP])]


TIED_N, TIED_SIZE, TIED_AT = 1200, 400, 600


TIED_EARLY = ((), (100,), (50, 100, 150))


def _tied_starts(seed, early):
    e = spiked(TIED_N, [], seed)
    e[TIED_AT: TIED_AT + 3] = 60.0, 20.0, 100.0
    for p in early:                                              # rows of earlier windows, so that the tied ones are not the first produced
        e[p: p + 2] = 50.0
    return e


@functools.lru_cache(maxsize=None)
def family_tied_starts():
    """Windows of 400 at every position, padding 0, values 60, 20, 100 at 600 .. 602.  The window that ends at 600 reports (600, 600), the
    next one (600, 601), and each of the 398 that hold the 100 as well reports (600, 600) and (602, 602), the 20 now below its
    threshold.  All start at 600 or touch: one merged row, whose first two rows in order of production weigh 0 and 1 -- in any other
    order of the tied starts the first two would almost surely weigh nothing.  Once alone, and behind the rows of one and of three
    two-point spikes that earlier windows report (a sort without its tie-break leaves the first rows of its input in place)."""
    segs = [pick(lambda sd: _tied_starts(sd, early), 1300, size=TIED_SIZE, step=1, pad=0) for early in TIED_EARLY]
    return [("tied starts",) + _call(segs, pad=0, sizes=[TIED_SIZE] * len(segs), steps=[1] * len(segs))]


EXACT_FAMILIES = ("cap", "signs_and_ties")


def all_calls():
    """(family, exact, calls) for every family of the sweep."""
    yield "tile_lengths", False, [c for pad in TILE_PADS for c in family_tile_lengths(pad)]
    yield "tile_offsets", False, [c for f in TILE_OFFSETS for c in family_tile_offsets(f)]
    yield "run_gaps", False, [c for pad in GAP_PADS for c in family_run_gaps(pad)]
    yield "sort_runs", False, [c for k in SORT_COUNTS for c in family_sort_runs(k)]
    yield "sort_merge", False, [c for k in (4096, 4097) for c in family_sort_merge(k)]
    yield "cap", True, family_cap()
    yield "degenerate", False, [c for lower in (False, True) for c in family_degenerate(lower)]
    yield "mixed", False, [c for k in (65, 129) for c in family_mixed(k)]
    yield "signs_and_ties", True, family_signs_and_ties()
    yield "covered_random", False, family_covered_random()
    yield "shoulders", False, family_shoulders()
    yield "far_carry", False, family_far_carry()
    yield "tied_starts", False, family_tied_starts()
