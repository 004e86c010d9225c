"""The statistics kernels of csrc/scoring.hip against exact references at their launch edges: the radix-selection quantiles, the centred
rolling mean, the two-level z-score, the quantile-trimmed critic z-score, and the segmented copies of all four.

What the older tests leave out (docs/history/scoring_statistics_sweep.md): the second pass of the quantile kernels' grid-stride loops
(more than 1 024 x 1 024 values), both sides of the candidate list's limit (4 095, 4 096, 4 097 values under one 33-bit key prefix) and
two routes in one call, the edges of stat_blocks (1 023 .. 1 025 and 262 143 .. 262 145 values, slices longer than four values a thread,
a merge tree over a count that is no power of two), statistics whose mean is large against their spread, the inclusive ends of the
trimmed mean on tied quartiles, the chunked rolling mean against a reference at origins other than 0, and the segmented copies against
anything but the single-signal call.

Everything goes through the C ABI.  Every output has one sentinel in front of it and one behind and is pre-filled with NaN -- with a
finite value where NaN is a legal result; every workspace is exactly as large as its *_workspace_bytes function says, filled with a
byte pattern, and followed by a guard of the same pattern that must be intact afterwards.  The references are tests/scoring_ref.py's
(exact sums, np.longdouble for the rest; pinned to oracle/scoring.py by tests/test_scoring_reference.py, which also shows on the CPU
that every input has the edge it is named for).  The allowances are counted from the kernel text (scoring_ref.rolling_additions,
stat_counts, zscore_allowance); quantiles are compared bit for bit.  Each test prints its worst error / allowance.
"""
import ctypes

import numpy as np
import pytest
import torch

import scoring_ref as sr
from test_gpu_scoring_sweep import FILL, _bits, _dev, _intact, _out, _quiet

pytestmark = pytest.mark.gpu

LD = sr.LD
GUARD, GUARD_BYTES = 0xA5, 256
F64 = torch.float64


class _Ws:
    """A workspace of exactly `nbytes` bytes with a guard behind it; all of it filled with the guard's pattern."""

    def __init__(self, nbytes):
        self.n = int(nbytes)
        self.buf = torch.full((self.n + GUARD_BYTES,), GUARD, dtype=torch.uint8, device="cuda")
        self.ptr = self.buf.data_ptr()

    def intact(self):
        return bool((self.buf[self.n:] == GUARD).all())


def _sync(*checks):
    torch.cuda.synchronize()
    for c in checks:
        assert c.intact() if isinstance(c, _Ws) else _intact(c)


def _at_offset_one(a):
    """The fp64 array on the device at a storage offset of one double (8 bytes past a 16-byte boundary)."""
    buf = torch.empty(len(a) + 1, dtype=F64, device="cuda")
    buf[1:].copy_(torch.from_numpy(np.ascontiguousarray(a)))
    v = buf[1:]
    assert v.data_ptr() % 16 == 8
    return v


# ------------------------------------------------------------------------------------------------ quantiles
def _quantiles(d, q):
    """hypad_quantiles of the device vector d (fp64) for the one or two q."""
    from hypad_amd import _C
    q = [float(v) for v in q]
    buf, out = _out(len(q), F64, FILL)
    ws = _Ws(_C.lib.hypad_quantile_workspace_bytes())
    qa = (ctypes.c_double * len(q))(*q)
    _C.check(_C.lib.hypad_quantiles(_C.ptr(d), d.numel(), qa, len(q), _C.ptr(out), ws.ptr, ws.n, _C.stream()), "quantiles")
    _sync(buf, ws)
    return out.cpu().numpy()


def _same_quantiles(got, ref, tag, sign_free=False):
    """Bit patterns equal (so the sign of a zero counts), NaN exactly where numpy has NaN.  sign_free: zeros of both signs in the input
    -- numpy's partition compares them equal and does not say which one it leaves at a rank."""
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    assert got.shape == ref.shape, tag
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, got, ref)
    if sign_free:
        assert np.array_equal(got[~nan], ref[~nan]), (tag, got, ref)
    else:
        assert np.array_equal(_bits(got)[~nan], _bits(ref)[~nan]), (tag, got, ref)


def _check_quantiles(x, qs, tag, offsets=(0, 1), sign_free=False):
    for off in offsets:
        d = _at_offset_one(x) if off else _dev(x, F64)
        for q in qs:
            _same_quantiles(_quantiles(d, q), _quiet(np.quantile, x, q), (tag, q, "offset", off), sign_free)
    return len(offsets) * len(qs)


@pytest.mark.parametrize("m", sr.BAND_SIZES)
def test_quantiles_at_the_edge_of_the_candidate_list(m):
    """m values under one 33-bit key prefix, 3 000 others: at 4 095 and 4 096 the quartiles and the median rank the candidate list (at
    4 096 a full one), at 4 097 and 8 192 they run the fall-back over the input; q = (0, 1) reads a list of two and a single key."""
    n = _check_quantiles(sr.band_input(m), sr.BAND_QS, ("band", m))
    print(f"\nstatistics sweep quantiles band m={m}: {n} calls, bits equal")


def test_quantiles_two_routes_in_one_call():
    """One quantile inside a band of 4 097 (fall-back), the other among scattered values (a list of two, or a single key): the four
    groups of qs_final run in lock step, and the group that is decided only keeps the barriers."""
    n = _check_quantiles(sr.band_input(4097, 1), sr.MIXED_QS, "mixed routes")
    print(f"\nstatistics sweep quantiles mixed routes: {n} calls, bits equal")


@pytest.fixture(scope="module")
def long_inputs():
    return {(f, n): sr.long_input(f, n) for f in ("normal", "fp32 origin", "band") for n in sr.LONG_NS}


@pytest.mark.parametrize("n", sr.LONG_NS)
@pytest.mark.parametrize("family", ["normal", "fp32 origin", "band"])
def test_quantiles_past_one_grid_pass(long_inputs, family, n):
    """More than 1 024 workgroups x 1 024 values: the level and compaction kernels take a second (and third) pass of their loop with
    the re-issued prefetch; the band family also runs the fall-back's own loop over all n values."""
    k = _check_quantiles(long_inputs[family, n], ((0.25, 0.75), (0.5,), (0.0, 1.0)), (family, n))
    print(f"\nstatistics sweep quantiles long {family} n={n}: {k} calls, bits equal")


@pytest.mark.parametrize("n", [1, 2, 5, 1024, 1025, 4097])
def test_quantiles_ranks_at_the_ends(n):
    rng = np.random.default_rng(n)
    x = rng.standard_normal(n)
    below1 = float(np.nextafter(1.0, 0.0))
    qs = [(0.0,), (1.0,), (below1,), (0.0, 1.0), (1.0, 0.0), (below1, 0.0), (0.5, 0.5), (1.0, 1.0), (0.0, 0.0), (0.25, 0.75)]
    if n > 1:
        qs += [(1.0 / (n - 1),), (1.0 / (n - 1), 1.0 - 1.0 / (n - 1))]
        exact = [k / (n - 1) for k in range(1, n - 1) if ((n - 1) * (k / (n - 1))).is_integer()][:: max(1, n // 7)]
        qs += [(q,) for q in exact] + ([(exact[0], exact[-1])] if exact else [])
    k = _check_quantiles(x, qs, ("ends", n))
    print(f"\nstatistics sweep quantiles ends n={n}: {k} calls, bits equal")


def test_quantiles_special_values(long_inputs):
    rng = np.random.default_rng(3)
    qs = ((0.25, 0.75), (0.5,), (0.0, 1.0), (0.1, 0.9))
    k = 0
    for name, x in (("+0.0 only", np.zeros(777)), ("-0.0 only", -np.zeros(777))):
        ref = np.quantile(x, (0.25, 0.75, 0.4))
        assert np.all(ref == 0)
        k += _check_quantiles(x, qs + ((0.4,),), name)
    both = np.where(rng.random(1001) < 0.5, 0.0, -0.0)
    k += _check_quantiles(both, qs, "zeros of both signs", sign_free=True)
    for name, x in (("+inf majority", np.concatenate([rng.standard_normal(300), [np.inf] * 900])),
                    ("-inf majority", np.concatenate([rng.standard_normal(300), [-np.inf] * 900])),
                    ("both infinities", np.concatenate([rng.standard_normal(100), [np.inf] * 500, [-np.inf] * 500])),
                    ("infinities only", np.concatenate([[np.inf] * 500, [-np.inf] * 501]))):
        rng.shuffle(x)
        k += _check_quantiles(x, qs, name)
    n = sr.LONG_NS[0]
    for where in (0, n - 1, 1024 * 1024 + 77):                # the first value, the last, one of the second grid pass
        x = long_inputs["normal", n].copy()
        x[where] = np.nan
        assert np.isnan(_quiet(np.quantile, x, (0.25, 0.75))).all()
        k += _check_quantiles(x, ((0.25, 0.75),), ("one NaN at", where))
    print(f"\nstatistics sweep quantiles special values: {k} calls, bits equal")


def _group_layout(rows, window):
    """(row_off, t_off) of a group with `rows` windows per segment (timestep layout: include/hypad.h)."""
    row_off = [0] + [int(v) for v in np.cumsum(rows)]
    return row_off, [r + s * (window - 1) for s, r in enumerate(row_off)]


@pytest.mark.parametrize("window", [1, 100])
def test_quantiles_signals_against_numpy_per_segment(long_inputs, window):
    """Three segments -- one crosses 1 048 576 timesteps, one holds a band of 4 097, one is a single window -- in two orders, against
    np.quantile of each segment (not against the single-signal call); a NaN in one segment makes that segment's row NaN, no other's."""
    from hypad_amd import _C
    series = {"long": long_inputs["normal", sr.LONG_NS[0]], "band": sr.band_input(4097, 1),
              "single": np.random.default_rng(window).standard_normal(window)}
    calls = 0
    for order in (("long", "band", "single"), ("single", "band", "long")):
        for poison in (None, "band"):
            segs = [series[k].copy() for k in order]
            if poison:
                segs[order.index(poison)][5] = np.nan
            rows = [len(s) - window + 1 for s in segs]
            row_off, t_off = _group_layout(rows, window)
            d = _dev(np.concatenate(segs), F64)
            assert d.numel() == t_off[-1]
            for q in ((0.25, 0.75), (0.5,), (0.01, 0.5)):
                buf, out = _out(3 * len(q), F64, FILL)
                ws = _Ws(_C.lib.hypad_quantiles_signals_workspace_bytes(3))
                qa = (ctypes.c_double * len(q))(*q)
                _C.check(_C.lib.hypad_quantiles_signals(_C.ptr(d), 3, _C.int64s(row_off), window, qa, len(q), _C.ptr(out), ws.ptr, ws.n,
                                                        _C.stream()), "quantiles_signals")
                _sync(buf, ws)
                got = out.cpu().numpy().reshape(3, len(q))
                for s, seg in enumerate(segs):
                    _same_quantiles(got[s], _quiet(np.quantile, seg, q), (order, poison, q, "segment", s))
                calls += 1
    print(f"\nstatistics sweep quantiles_signals window={window}: {calls} calls, bits equal")


# ------------------------------------------------------------------------------------------------ z-score and critic z-score
def _stats_ws():
    from hypad_amd import _C
    return _Ws(_C.STATS_WORKSPACE_BYTES)


def _zscore(d):
    from hypad_amd import _C
    buf, out = _out(d.numel(), F64, FILL)
    ws = _stats_ws()
    _C.check(_C.lib.hypad_zscore_clip(_C.ptr(d), _C.ptr(out), d.numel(), ws.ptr, ws.n, _C.stream()), "zscore_clip")
    _sync(buf, ws)
    return out.cpu().numpy()


def _critic_zscore(d, lo, hi):
    from hypad_amd import _C
    buf, out = _out(d.numel(), F64, FILL)
    ws = _stats_ws()
    _C.check(_C.lib.hypad_critic_zscore(_C.ptr(d), float(lo), float(hi), _C.ptr(out), d.numel(), ws.ptr, ws.n, _C.stream()), "critic_zscore")
    _sync(buf, ws)
    return out.cpu().numpy()


def _critic_score(d):
    from hypad_amd import _C
    buf, out = _out(d.numel(), F64, FILL)
    ws = _Ws(_C.lib.hypad_critic_score_workspace_bytes())
    _C.check(_C.lib.hypad_critic_score(_C.ptr(d), _C.ptr(out), d.numel(), ws.ptr, ws.n, _C.stream()), "critic_score")
    _sync(buf, ws)
    return out.cpu().numpy()


def _ratio(got, ref, allow, tag):
    """max |got - ref| / allow with ref in np.longdouble; NaN exactly where the reference has NaN; asserts it is at most 1."""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN at", np.flatnonzero(np.isnan(got) != nan)[:8])
    if nan.all():
        return 0.0
    err = np.abs(got[~nan].astype(LD) - ref[~nan]).astype(np.float64)
    allow = np.broadcast_to(np.asarray(allow, dtype=np.float64), got.shape)[~nan]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / allow)
    i = int(np.argmax(ratio))
    assert ratio[i] <= 1.0, (tag, "element", int(np.flatnonzero(~nan)[i]), "error", err[i], "allowance", allow[i])
    return float(ratio[i])


def _check_statistics(x, tag):
    """hypad_zscore_clip, hypad_critic_zscore (fed np.quantile's quartiles) and hypad_critic_score of x: (worst z-score ratio, worst
    critic ratio); hypad_critic_score has hypad_critic_zscore's bits."""
    d = _dev(x, F64)
    moments = sr.exact_moments(x)
    zref = sr.zscore_exact(x, moments)
    za = sr.zscore_allowance(x, zref, *moments) if not np.isnan(zref).all() else 0.0
    wz = _ratio(_zscore(d), zref, za, (tag, "zscore_clip"))
    lo, hi = _quiet(np.quantile, x, (0.25, 0.75))
    cref, tmean = sr.critic_zscore_exact(x, lo, hi, moments, with_mean=True)
    ca = sr.zscore_allowance(x, cref, tmean, moments[1], trimmed=True) if not np.isnan(cref).all() else 0.0
    got = _critic_zscore(d, lo, hi)
    wc = _ratio(got, cref, ca, (tag, "critic_zscore"))
    fused = _critic_score(d)
    assert np.array_equal(_bits(fused), _bits(got)) or (np.isnan(fused).all() and np.isnan(got).all()), (tag, "critic_score")
    return wz, wc


@pytest.mark.parametrize("t", sr.STAT_TS)
def test_zscore_and_critic_zscore_every_family(t):
    """Every edge of stat_blocks and of the slice length, seven families each: well-conditioned, a mean 10^6 spreads away, a ramp whose
    slice means differ by more than the spread inside a slice (the merge term carries the variance), and the three that are NaN
    everywhere (a constant: 0 / 0; a NaN in the last slice; one +inf)."""
    worst = {}
    for family in sr.STAT_FAMILIES:
        x = sr.stat_input(family, t)
        worst[family] = _check_statistics(x, (family, t))
        if family in ("constant", "nan in the last slice", "one +inf") or t == 1:
            assert np.isnan(sr.zscore_exact(x)).all(), (family, t)          # (so _ratio has held the kernel to NaN everywhere)
    print(f"\nstatistics sweep z-score / critic t={t}: worst error / allowance " + ", ".join(f"{k} {a:.3f} / {b:.3f}" for k, (a, b) in worst.items()))


@pytest.mark.parametrize("n", sr.TIED_NS)
def test_trimmed_mean_takes_both_tied_ends(n):
    """n = 1 (mod 4), values of two decimals: the quartiles are samples that at least 20 values equal; `x >= lo && x <= hi` keeps them
    all.  Dropping the ties of one end moves the mean by more than 10^6 allowances (tests/test_scoring_reference.py)."""
    x = sr.tied_input(n)
    lo, hi, nlo, nhi = sr.ties_at_quartiles(x)
    assert nlo >= sr.MIN_TIES and nhi >= sr.MIN_TIES and (x == lo).any() and (x == hi).any()
    wz, wc = _check_statistics(x, ("tied", n))
    print(f"\nstatistics sweep trimmed mean n={n}: {nlo} / {nhi} values on the quartiles, worst error / allowance {wz:.3f} / {wc:.3f}")


# ------------------------------------------------------------------------------------------------ rolling mean
def _rolling(d, w, origin, sub=None):
    """hypad_rolling_mean of the device series d (fp64) at `origin`, the workspace exactly as large as asked for (none at w <= 32)."""
    from hypad_amd import _C
    t = d.numel()
    buf, out = _out(t, F64, FILL)
    ws = _Ws(_C.lib.hypad_rolling_workspace_bytes(t)) if w > sr.ROLL_DIRECT_MAX else None
    _C.check(_C.lib.hypad_rolling_mean(_C.ptr(d), _C.ptr(sub), _C.ptr(out), t, w, origin, ws.ptr if ws else None, ws.n if ws else 0, _C.stream()),
             "rolling_mean")
    _sync(buf, *([ws] if ws else []))
    return out.cpu().numpy()


_ROLL_REFS = {}


def _roll_ref(key, x, w, sub=None):
    """(exact rolling mean, allowance) of one input, computed once per module."""
    if key not in _ROLL_REFS:
        _ROLL_REFS[key] = (sr.rolling_mean_exact_long(x, w, sub), sr.rolling_allowance(x, w, sub))
    return _ROLL_REFS[key]


@pytest.mark.parametrize("w", sr.ROLL_WS)
def test_rolling_mean_short_series_every_origin(w):
    """T = 1, w / 2 - 1, w / 2, w - 1, w, w + 1, 600 x ten origins x four NaN layouts (the runs placed for origin 0: at the others they
    straddle the chunk boundaries); NaN exactly where pandas has NaN.  At origin 0 and 17 also with the fused subtrahend, whose NaN
    are values the window skips: the bits of the rolling mean of the materialised |in - sub|."""
    worst = 0.0
    rng = np.random.default_rng(w)
    for t in sr.roll_short_ts(w):
        for layout in ("none", "scattered", "run 16 aligned", "min periods"):
            if not sr.layout_fits(t, w, 0, layout):         # (min periods: T = 600 up to w = 257; w = 1 250 has it in the long test)
                continue
            x = sr.roll_input(t, w, 0, layout)
            ref, allow = _roll_ref((t, w, layout), x, w)
            d = _dev(x, F64)
            for origin in sr.ROLL_ORIGINS:
                worst = max(worst, _ratio(_rolling(d, w, origin), ref, allow, (w, t, layout, origin)))
        x = sr.roll_input(t, w, 0, "none")
        sub = (x + 0.1 * rng.standard_normal(t)).astype(np.float32)
        sub[rng.integers(0, t, max(1, t // 50))] = np.nan
        ref, allow = _roll_ref((t, w, "sub"), x, w, sub)
        d, ds = _dev(x, F64), _dev(sub, torch.float32)
        plain = _dev(sr.rolling_values(x, sub), F64)
        for origin in (0, 17):
            fused = _rolling(d, w, origin, ds)
            assert np.array_equal(_bits(fused), _bits(_rolling(plain, w, origin))), (w, t, origin, "fused subtrahend")
            worst = max(worst, _ratio(fused, ref, allow, (w, t, "sub", origin)))
    print(f"\nstatistics sweep rolling mean short w={w}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("w,origin", sr.ROLL_LONG_PAIRS)
def test_rolling_mean_long_series_every_layout(w, origin):
    """T = 4 095, 4 096, 4 097 (a second workgroup of the chunk sums), 6 000 at every NaN layout, the runs on the absolute chunk
    boundaries of this origin: emptied 16- and 256-chunks, a run of 600, windows that meet min_periods exactly beside windows that
    miss it by one."""
    worst = 0.0
    for t in sr.ROLL_LONG_TS:
        for layout in sr.ROLL_LAYOUTS:
            x = sr.roll_input(t, w, origin, layout)
            ref, allow = _roll_ref((t, w, layout, origin % 256), x, w)
            worst = max(worst, _ratio(_rolling(_dev(x, F64), w, origin), ref, allow, (w, t, layout, origin)))
    print(f"\nstatistics sweep rolling mean long w={w} origin={origin}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("w", [7, 33, 257, 1250])
def test_rolling_mean_of_a_slice_has_the_bits_of_the_whole_at_chunk_edges(w):
    """The slice [a, b) smoothed at origin O + a equals the whole series smoothed at origin O, bit for bit, at every timestep whose
    window lies inside the slice -- a and b at and around multiples of 16 and 256, O every origin of the sweep."""
    t = 6000
    x = sr.roll_input(t, w, 0, "scattered", seed=3)
    d = _dev(x, F64)
    off = (w - 1) // 2
    cuts = [(a, b) for a in (0, 15, 16, 17, 255, 256, 257, 1024) for b in (a + 2 * w + 40, 4095, 4096, 4097, t) if b - a >= w + 2 and b <= t]
    n = 0
    for origin in sr.ROLL_ORIGINS:
        whole = _rolling(d, w, origin)
        for a, b in cuts[origin % 3:: 3] + cuts[:2]:
            part = _rolling(d[a:b].contiguous(), w, origin + a)
            first = 0 if a == 0 else w - 1 - off             # local timesteps [first, last]: the window is not clipped by the slice
            last = b - a - 1 if b == t else b - a - 1 - off
            assert np.array_equal(_bits(part[first:last + 1]), _bits(whole[a + first: a + last + 1])), (w, origin, a, b)
            n += 1
    print(f"\nstatistics sweep rolling mean slices w={w}: {n} slices, bits equal")


# ------------------------------------------------------------------------------------------------ segmented copies
SEG_ROWS = (99, 100, 3299, 3300, 5000)                      # trunc(n 0.01) = 0, 1, 32, 33, 50
SEG_ORDERS = ((0, 1, 2, 3, 4), (4, 2, 0, 3, 1))


def _after_rolling(unsmoothed, in_allow, w):
    """(reference, allowance) of the rolling mean of a series known as `unsmoothed` (np.longdouble) to within `in_allow` per element:
    a mean of values each off by at most max(in_allow) is off by at most that, the fp64 series handed to the exact rolling mean by one
    more rounding, and the kernel's own summation by the rolling allowance."""
    x64 = unsmoothed.astype(np.float64)
    if w == 0 or np.isnan(x64).all():
        return np.full(len(x64), np.nan, dtype=LD), 0.0
    feed = float(np.max(in_allow + sr.U * np.abs(x64)))
    return sr.rolling_mean_exact_long(x64, w), sr.rolling_allowance(x64, w) + feed


def _after_zscore(smoothed, in_allow):
    """(reference, allowance) of zscore_clip of a series known as `smoothed` (np.longdouble) to within `in_allow`: with every value off
    by at most e = max(in_allow) the mean moves by at most e and the standard deviation by at most e (the norm of the deviations moves
    by at most the norm of the perturbation), so z moves by at most (in_allow + e) / sd + |z| e / sd."""
    x64 = smoothed.astype(np.float64)
    if np.isnan(x64).any():
        return np.full(len(x64), np.nan, dtype=LD), 0.0
    mean, sd = sr.exact_moments(x64)
    ref = sr.zscore_exact(x64, (mean, sd))
    e = float(np.max(in_allow + sr.U * np.abs(x64)))
    z = np.abs(x64 - float(mean)) / float(sd)
    return ref, sr.zscore_allowance(x64, ref, mean, sd) + (in_allow + sr.U * np.abs(x64) + e + z * e) / float(sd)


_SEG_SERIES = {}


def _seg_series(n, window, nan_run=None):
    """One segment's (true series fp64, medians fp32) of n windows, and the references of its three kinds -- once per module.
    nan_run = (a, b): the true series is NaN on [a, b), so the point-wise error is NaN there and the area and DTW errors around it."""
    key = (n, window, nan_run)
    if key not in _SEG_SERIES:
        from hypad_amd import _C
        t = n + window - 1
        rng = np.random.default_rng(1000 * n + window)
        y = np.sin(np.arange(t) / 9.0) + 0.2 * rng.standard_normal(t)
        yh = (y + 0.1 * rng.standard_normal(t) * (1.0 + (np.arange(t) % 400 < 30))).astype(np.float32)
        if nan_run:
            y[nan_run[0]: nan_run[1]] = np.nan
        w = int(n * 0.01)
        errs = {"point": np.abs(y - yh.astype(np.float64))}
        dy, dh = _dev(y, F64), _dev(yh, torch.float32)
        for kind, fn in (("area", _C.lib.hypad_area_error), ("dtw", _C.lib.hypad_dtw_error)):      # (the error series are the earlier sweep's)
            buf, out = _out(t, F64)
            _C.check(fn(_C.ptr(dy), _C.ptr(dh), _C.ptr(out), t, 10, _C.stream()), kind)
            _sync(buf)
            errs[kind] = out.cpu().numpy()
        refs = {}
        for kind, e in errs.items():
            if w == 0:
                refs[kind] = (np.full(t, np.nan, dtype=LD), 0.0)
            else:
                refs[kind] = _after_zscore(sr.rolling_mean_exact_long(e, w), sr.rolling_allowance(e, w))
        _SEG_SERIES[key] = (y, yh, refs)
    return _SEG_SERIES[key]


@pytest.mark.parametrize("order", SEG_ORDERS)
@pytest.mark.parametrize("window", [100, 3])
def test_rec_scores_signals_against_the_references_per_segment(window, order):
    """All three kinds in one call (blockIdx.z), five segments whose smoothing windows are 0 (all NaN), 1, 32, 33 (the direct and the
    chunked form side by side) and 50, at timestep offsets on and off the multiples of 16 and 256: every kind of every segment within
    the allowance of the exact rolling mean followed by the exact z-score of that kind's own error series."""
    from hypad_amd import _C
    rows = [SEG_ROWS[i] for i in order]
    assert [int(n * 0.01) for n in SEG_ROWS] == [0, 1, 32, 33, 50]
    row_off, t_off = _group_layout(rows, window)
    segs = [_seg_series(n, window) for n in rows]
    dy, dh = _dev(np.concatenate([s[0] for s in segs]), F64), _dev(np.concatenate([s[1] for s in segs]), torch.float32)
    offs = _C.int64s(row_off)
    outs = {k: _out(t_off[-1], F64, FILL) for k in ("point", "area", "dtw")}
    ws = _Ws(_C.lib.hypad_rec_scores_signals_workspace_bytes(len(rows), offs, window))
    _C.check(_C.lib.hypad_rec_scores_signals(7, _C.ptr(dy), _C.ptr(dh), _C.ptr(outs["point"][1]), _C.ptr(outs["area"][1]), _C.ptr(outs["dtw"][1]),
                                             len(rows), offs, window, 10, ws.ptr, ws.n, _C.stream()), "rec_scores_signals")
    _sync(ws, *[b for b, _ in outs.values()])
    worst = {}
    for kind, (_, out) in outs.items():
        got = out.cpu().numpy()
        worst[kind] = max(_ratio(got[t_off[s]: t_off[s + 1]], *segs[s][2][kind], (kind, window, "segment", s, rows[s])) for s in range(len(rows)))
        assert np.isnan(got[t_off[rows.index(99)]: t_off[rows.index(99) + 1]]).all()
    print(f"\nstatistics sweep rec_scores_signals window={window} order={order}: worst error / allowance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _wide_rows(window):
    """A small segment and two whose smoothing windows (600, 601) hold whole 256-chunks: 60 000 windows (a partial last 256-chunk) and
    as many as make 60 160 = 235 x 256 timesteps (a full last 256-chunk, which the clipped windows at the segment's end read)."""
    rows = [100, 60000, 60160 - (window - 1)]
    assert (rows[1] + window - 1) % 256 not in (0, 255) and (rows[2] + window - 1) % 256 == 0 and int(rows[2] * 0.01) >= 511
    return rows


@pytest.mark.parametrize("window", [100, 3])
def test_rec_scores_signals_with_a_window_over_whole_256_chunks(window):
    """Two segments of about 60 000 windows behind a small one: the smoothing window of 600 reads the level-2 (256-chunk) sums of the
    segmented kernels, which no window up to 50 does.  The first one's last 256-chunk is partial (60 099 and 60 002 timesteps), the
    second one's is full (60 160 timesteps) and is read by the windows that the segment's end clips.  The first one's true series is
    NaN on the aligned run [512, 768), which empties one 256-chunk of the point-wise error (and, with the values around it, of the area
    and DTW errors); every window keeps at least w // 2 = 300 valid values."""
    from hypad_amd import _C
    rows = _wide_rows(window)
    row_off, t_off = _group_layout(rows, window)
    segs = [_seg_series(rows[0], window), _seg_series(rows[1], window, (512, 768)), _seg_series(rows[2], window)]
    perr = np.abs(segs[1][0] - segs[1][1].astype(np.float64))
    assert sr.empty_chunks(perr, 0, 256) == 1 and sr.window_counts(perr, 600).min() >= 300      # (300 only where the series' ends clip the window)
    dy, dh = _dev(np.concatenate([s[0] for s in segs]), F64), _dev(np.concatenate([s[1] for s in segs]), torch.float32)
    offs = _C.int64s(row_off)
    outs = {k: _out(t_off[-1], F64, FILL) for k in ("point", "area", "dtw")}
    ws = _Ws(_C.lib.hypad_rec_scores_signals_workspace_bytes(3, offs, window))
    _C.check(_C.lib.hypad_rec_scores_signals(7, _C.ptr(dy), _C.ptr(dh), _C.ptr(outs["point"][1]), _C.ptr(outs["area"][1]), _C.ptr(outs["dtw"][1]),
                                             3, offs, window, 10, ws.ptr, ws.n, _C.stream()), "rec_scores_signals")
    _sync(ws, *[b for b, _ in outs.values()])
    worst = {}
    for kind, (_, out) in outs.items():
        got = out.cpu().numpy()
        assert not np.isnan(got[t_off[1]: t_off[2]]).any(), kind
        worst[kind] = max(_ratio(got[t_off[s]: t_off[s + 1]], *segs[s][2][kind], (kind, window, "segment", s, rows[s])) for s in range(3))
    print(f"\nstatistics sweep rec_scores_signals wide window={window}: worst error / allowance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


def _critic_tail_ref(modes, w):
    """(reference, allowance) of hypad_critic_score followed by the rolling mean of window w on one segment's modes."""
    lo, hi = np.quantile(modes, (0.25, 0.75))
    moments = sr.exact_moments(modes)
    c, tmean = sr.critic_zscore_exact(modes, lo, hi, moments, with_mean=True)
    if np.isnan(c).all():
        return np.full(len(modes), np.nan, dtype=LD), 0.0
    return _after_rolling(c, sr.zscore_allowance(modes, c, tmean, moments[1], trimmed=True), w)


@pytest.mark.parametrize("order", SEG_ORDERS)
@pytest.mark.parametrize("window", [100, 3])
def test_critic_score_signals_against_the_references_per_segment(window, order):
    from hypad_amd import _C
    rows = [SEG_ROWS[i] for i in order]
    row_off, t_off = _group_layout(rows, window)
    segs = [np.random.default_rng(n + window).standard_normal(n + window - 1).astype(np.float32).astype(np.float64) + 0.25 for n in rows]
    d = _dev(np.concatenate(segs), F64)
    offs = _C.int64s(row_off)
    buf, out = _out(t_off[-1], F64, FILL)
    ws = _Ws(_C.lib.hypad_critic_score_signals_workspace_bytes(len(rows), offs, window))
    _C.check(_C.lib.hypad_critic_score_signals(_C.ptr(d), _C.ptr(out), len(rows), offs, window, ws.ptr, ws.n, _C.stream()), "critic_score_signals")
    _sync(buf, ws)
    got = out.cpu().numpy()
    worst = max(_ratio(got[t_off[s]: t_off[s + 1]], *_critic_tail_ref(segs[s], int(rows[s] * 0.01)), (window, "segment", s, rows[s]))
                for s in range(len(rows)))
    print(f"\nstatistics sweep critic_score_signals window={window} order={order}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("window", [100, 3])
def test_critic_score_signals_with_a_window_over_whole_256_chunks(window):
    """The two wide segments of _wide_rows (smoothing windows 600 and 601; a partial and a full last 256-chunk).  (A NaN among the modes
    makes the whole segment NaN through its quantiles: no chunk of this chain can be emptied.)"""
    from hypad_amd import _C
    rows = _wide_rows(window)
    row_off, t_off = _group_layout(rows, window)
    segs = [np.random.default_rng(n + window).standard_normal(n + window - 1).astype(np.float32).astype(np.float64) + 0.25 for n in rows]
    offs = _C.int64s(row_off)
    buf, out = _out(t_off[-1], F64, FILL)
    ws = _Ws(_C.lib.hypad_critic_score_signals_workspace_bytes(3, offs, window))
    _C.check(_C.lib.hypad_critic_score_signals(_C.ptr(_dev(np.concatenate(segs), F64)), _C.ptr(out), 3, offs, window, ws.ptr, ws.n, _C.stream()),
             "critic_score_signals")
    _sync(buf, ws)
    got = out.cpu().numpy()
    worst = max(_ratio(got[t_off[s]: t_off[s + 1]], *_critic_tail_ref(segs[s], int(rows[s] * 0.01)), (window, "segment", s, rows[s])) for s in range(3))
    print(f"\nstatistics sweep critic_score_signals wide window={window}: worst error / allowance {worst:.3f}")


def test_critic_chain_signals_tail_with_tied_quartiles_across_the_launch_chunks():
    """66 segments (two of about 60 000 windows, whose smoothing windows hold whole 256-chunks, the last one partial and full): the launches take
    64 at a time, and segments 63, 64 and 65 -- the last of the first chunk, the first two of the
    second -- have 4 097 timesteps (1 mod 4) of critic values with one decimal, so that their modes' quartiles are heavily tied
    samples.  The output of every segment is held to the references of its own modes (modes_out): the trimmed critic z-score with both
    ends inclusive, then the rolling mean of the segment's own window."""
    from hypad_amd import _C
    window = 5
    rng = np.random.default_rng(66)
    rows = [int(v) for v in rng.integers(60, 420, 66)]
    rows[63] = rows[64] = rows[65] = 4097 - (window - 1)
    rows[0], rows[7] = 99, 100
    rows[30], rows[31] = _wide_rows(window)[1:]              # smoothing windows 600 and 601: the 256-chunk sums of the segmented rolling mean are read
    row_off, t_off = _group_layout(rows, window)
    critic = rng.standard_normal(row_off[-1]).astype(np.float32)
    for s in (63, 64, 65):
        critic[row_off[s]: row_off[s + 1]] = np.round(critic[row_off[s]: row_off[s + 1]] * 10) / 10
    offs = _C.int64s(row_off)
    mbuf, modes = _out(t_off[-1], F64)
    obuf, out = _out(t_off[-1], F64, FILL)
    ws = _Ws(_C.lib.hypad_critic_chain_signals_workspace_bytes(66, offs, window))
    _C.check(_C.lib.hypad_critic_chain_signals(_C.ptr(_dev(critic, torch.float32)), _C.ptr(modes), _C.ptr(out), 66, offs, window, ws.ptr, ws.n,
                                               _C.stream()), "critic_chain_signals")
    _sync(mbuf, obuf, ws)
    modes, got = modes.cpu().numpy(), out.cpu().numpy()
    assert not np.isnan(modes).any()
    worst = 0.0
    for s in range(66):
        m = modes[t_off[s]: t_off[s + 1]]
        if s in (63, 64, 65):
            lo, hi, nlo, nhi = sr.ties_at_quartiles(m)
            assert len(m) % 4 == 1 and nlo >= sr.MIN_TIES and nhi >= sr.MIN_TIES, (s, nlo, nhi)
        worst = max(worst, _ratio(got[t_off[s]: t_off[s + 1]], *_critic_tail_ref(m, int(rows[s] * 0.01)), ("segment", s, rows[s])))
    assert np.isnan(got[t_off[0]: t_off[1]]).all() and not np.isnan(got[t_off[7]: t_off[8]]).any()
    print(f"\nstatistics sweep critic_chain_signals: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("in_place", [False, True])
def test_zscore_clip_signals_against_the_reference_per_segment(in_place):
    """Segments of 1 (NaN), 1 024, 1 025 and 262 145 values and 65 of 1 .. 40 values -- 69 segments, two launch chunks -- out of place and
    in place (in == out), each against the exact z-score of the segment alone."""
    from hypad_amd import _C
    rng = np.random.default_rng(69)
    sizes = [int(v) for v in rng.integers(1, 41, 30)] + [1, 1024] + [int(v) for v in rng.integers(1, 41, 33)] + [1025, 262145, 1, 2]
    assert len(sizes) == 69
    seg_off = [0] + [int(v) for v in np.cumsum(sizes)]
    segs = [5.0 + 2.0 * rng.standard_normal(n) + (1e6 if i % 5 == 0 else 0.0) for i, n in enumerate(sizes)]
    x = np.concatenate(segs)
    buf, io = _out(len(x), F64, FILL)
    if in_place:
        io.copy_(torch.from_numpy(x))
    src = io if in_place else _dev(x, F64)
    ws = _Ws(_C.lib.hypad_zscore_clip_signals_workspace_bytes(69))
    _C.check(_C.lib.hypad_zscore_clip_signals(_C.ptr(src), _C.ptr(io), 69, _C.int64s(seg_off), ws.ptr, ws.n, _C.stream()), "zscore_clip_signals")
    _sync(buf, ws)
    got = io.cpu().numpy()
    worst = 0.0
    for s, seg in enumerate(segs):
        moments = sr.exact_moments(seg)
        ref = sr.zscore_exact(seg, moments)
        allow = sr.zscore_allowance(seg, ref, *moments) if not np.isnan(ref).all() else 0.0
        worst = max(worst, _ratio(got[seg_off[s]: seg_off[s + 1]], ref, allow, ("segment", s, sizes[s], in_place)))
    assert all(np.isnan(got[seg_off[s]]) for s, n in enumerate(sizes) if n == 1)
    print(f"\nstatistics sweep zscore_clip_signals in_place={in_place}: worst error / allowance {worst:.3f}")
