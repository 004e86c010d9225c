"""The single-signal scoring kernels of csrc/scoring.hip against oracle/scoring.py at every launch edge.

Since the bodies of the un-roll, DTW, KDE and quantile kernels are one text shared by the single-signal and the segmented kernel, "the
segmented launch has the single-signal launch's bits" says nothing about a defect in a body.  This file holds the single-signal
kernels themselves to the reference: every window class of hypad_unroll_median at both edges with interior tiles, every outcome of its
two-pivot filter (tests/scoring_ref.py models the decision; tests/test_scoring_reference.py checks on the CPU that the inputs used
here reach each outcome), NaN, the second iteration of its tile loop; every instantiation of hypad_dtw_error; hypad_area_error at odd
and short windows; the KDE mode at the edges of its window classes and past one grid pass; row norms and the ten combinations; and
the grid-stride loops of the point / area / DTW / rolling kernels (a series of 2 097 452 timesteps: one element past 8 192 x 256).

Everything goes through the C ABI.  Every output has one sentinel in front of it and one behind and is pre-filled with NaN -- with a
finite value where NaN is a legal result.  Each test prints its worst observed error / allowance (docs/history/scoring_kernels_sweep.md).
"""
import warnings

import numpy as np
import pytest
import torch

import scoring_ref as sr
from sweep_common import Checker, _at_offset

pytestmark = pytest.mark.gpu

NAN = float("nan")
SENT = 12345.0
FILL = -777.25                       # pre-fill where NaN is a legal result
LONG_T = 8192 * 256 + 300            # one grid pass of the 256-thread elementwise kernels, and 300 more


def _out(n, dtype, fill=NAN):
    buf = torch.full((n + 2,), fill, dtype=dtype, device="cuda")
    buf[0] = SENT
    buf[-1] = SENT
    return buf, buf[1:-1]


def _intact(*bufs):
    return all(b is None or (float(b[0]) == SENT and float(b[-1]) == SENT) for b in bufs)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", dtype).contiguous()


def _quiet(fn, *args):
    """fn(*args) without numpy's warnings about NaN, overflow and inf - inf (the cases that are there to produce them)."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn(*args)


# ------------------------------------------------------------------------------------------------ un-roll median
def _unroll(yh, summary, fill=NAN):
    """hypad_unroll_median on the device matrix yh: (median float32 (T,), summary float64 (T, 5) or None) as NumPy arrays."""
    from hypad_amd import _C
    n, w = yh.shape
    t = n + w - 1
    mb, med = _out(t, torch.float32, fill)
    sb, summ = _out(5 * t, torch.float64, fill) if summary else (None, None)
    _C.check(_C.lib.hypad_unroll_median(_C.ptr(yh), _C.ptr(med), _C.ptr(summ), n, w, _C.stream()), "unroll_median")
    torch.cuda.synchronize()
    assert _intact(mb, sb), (n, w, summary)
    return med.cpu().numpy(), (summ.cpu().numpy().reshape(t, 5) if summary else None)


def _oracle_unroll(y):
    from oracle import scoring as osc
    med, summ = _quiet(osc.unroll_predictions, y, True)
    return med, summ.reshape(-1, 5)


def _same_medians(got, ref, tag):
    """Bit-equal (the sign of a zero included), NaN exactly where the reference has NaN."""
    assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape, tag
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN at", np.flatnonzero(np.isnan(got) != nan)[:8])
    bad = np.flatnonzero(~nan & (_bits(got) != _bits(ref)))
    assert not len(bad), (tag, "median differs at", bad[:8], got[bad[:8]], ref[bad[:8]])


def _same_summary(summ, med, ref, tag, sign_free=None):
    """min and max bit-equal, p50 the median, p25 / p75 within 1e-6 max(1, |ref|); all five NaN where the reference is NaN.  Returns
    the worst |p25 / p75 error| / allowance."""
    nan = np.isnan(ref[:, 0])
    assert np.array_equal(np.isnan(summ), np.repeat(nan[:, None], 5, axis=1)), (tag, "NaN positions of the summary")
    ok = ~nan
    strict = ok if sign_free is None else ok & ~sign_free
    for col, name in ((0, "min"), (4, "max")):
        bad = np.flatnonzero(strict & (_bits(summ[:, col]) != _bits(ref[:, col])))
        assert not len(bad), (tag, name, bad[:8], summ[bad[:8], col], ref[bad[:8], col])
        assert np.array_equal(summ[ok, col], ref[ok, col]), (tag, name)
    # p50 is the median -- wherever the reference's own p50 is its median: np.percentile(v, 50) of an even count is a + (b - a) / 2 taken
    # from the upper value, np.median is (a + b) / 2, and in float32 the two differ by an ulp on ~7 % of random diagonals.  There p50 is
    # held to the reference's p50 like p25 and p75.
    same = ok & (ref[:, 2] == med.astype(np.float64))
    bad = np.flatnonzero(same & (summ[:, 2] != med.astype(np.float64)))
    assert not len(bad), (tag, "p50 is not the median at", bad[:8], summ[bad[:8], 2], med[bad[:8]])
    worst = 0.0
    for col in (1, 2, 3):
        ratio = np.abs(summ[ok, col] - ref[ok, col]) / (1e-6 * np.maximum(1.0, np.abs(ref[ok, col])))
        if ratio.size:
            assert not np.isnan(ratio).any() and ratio.max() <= 1.0, (tag, "p%d" % (25 * col), int(np.argmax(ratio)), ratio.max())
            worst = max(worst, float(ratio.max()))
    return worst


def _check_unroll(y, tag, summaries=(False, True), offset=0, fill=NAN, sign_free=None, ref=None):
    """hypad_unroll_median of the float32 matrix y, medians only and with the summary, against the oracle.  sign_free: the timesteps
    at which the minimum and the maximum are zeros whose sign numpy does not determine."""
    ref_med, ref_sum = ref if ref is not None else _oracle_unroll(y)
    d = _at_offset(torch.from_numpy(y), offset) if offset else _dev(y, torch.float32)
    worst = 0.0
    for s in summaries:
        med, summ = _unroll(d, s, fill)
        _same_medians(med, ref_med, (tag, "summary" if s else "medians only"))
        if s:
            worst = max(worst, _same_summary(summ, med, ref_sum, tag, sign_free))
    return worst


UNROLL_WINDOWS = (1, 2, 3, 4, 5, 63, 64, 65, 100, 127, 128, 129, 255, 256)


@pytest.mark.parametrize("w", UNROLL_WINDOWS)
def test_unroll_every_window_class_with_interior_tiles(w):
    """n = W + 300: a clipped first tile, at least one interior 128-timestep tile, a clipped last tile that is not full; at W = 100 and
    129 also the short series around the window and around one tile."""
    rng = np.random.default_rng(w)
    n = w + 300
    assert (w - 1 + 127) // 128 * 128 + 128 <= n and (n + w - 1) % 128 != 0          # an interior tile exists; the last tile is partial
    y = rng.standard_normal((n, w)).astype(np.float32)
    y[rng.integers(0, n), rng.integers(0, w)] = y[0, 0]
    worst = _check_unroll(y, (n, w))
    if w in (100, 129):
        for n in (1, 2, w - 1, w, w + 1, 127, 128, 129):
            worst = max(worst, _check_unroll(rng.standard_normal((n, w)).astype(np.float32), (n, w)))
    print(f"\nscoring sweep unroll W={w}: worst quartile error / allowance {worst:.3f}")


@pytest.mark.parametrize("w", [100, 129])
def test_unroll_at_storage_offset_one(w):
    rng = np.random.default_rng(w + 1)
    worst = 0.0
    for n in (w + 300, 1, 2, w - 1, w, w + 1, 127, 128, 129):
        worst = max(worst, _check_unroll(rng.standard_normal((n, w)).astype(np.float32), (n, w, "offset 1"), offset=1))
    print(f"\nscoring sweep unroll offset 1 W={w}: worst quartile error / allowance {worst:.3f}")


@pytest.mark.parametrize("w", sr.FILTER_WINDOWS)
def test_unroll_every_outcome_of_the_filter(w):
    """The input families of tests/scoring_ref.py: each sends at least 20 timesteps of the medians-only launch down one outcome of
    the filter -- hit, pivots miss, more than 64 candidates, ties among the candidates (tests/test_scoring_reference.py asserts it
    with the model of the decision)."""
    worst = 0.0
    for name in sr.FAMILIES:
        worst = max(worst, _check_unroll(sr.family(name, w), (name, w)))
    print(f"\nscoring sweep unroll filter W={w}: worst quartile error / allowance {worst:.3f}")


def _zero_sign_free(y):
    """Timesteps whose anti-diagonal holds zeros of both signs: numpy's median, minimum and maximum may be either zero."""
    from oracle import scoring as osc
    n, w = y.shape
    out = np.zeros(n + w - 1, dtype=bool)
    for t in range(n + w - 1):
        v = osc.antidiagonal(y, t)
        z = np.signbit(v[v == 0])
        out[t] = z.any() and not z.all()
    return out


@pytest.mark.parametrize("w", [64, 100, 129])
def test_unroll_special_values(w):
    rng = np.random.default_rng(w + 2)
    n = w + 140
    base = rng.standard_normal((n, w)).astype(np.float32)
    # all-equal rows: every anti-diagonal is a set of different values, one per row
    rows = np.repeat(rng.standard_normal((n, 1)).astype(np.float32), w, axis=1)
    worst = _check_unroll(rows, ("equal rows", w))
    # zeros of both signs, alone and among other values, and negative zeros alone among values.  A median that is a zero is +0.0, as
    # numpy's is: it takes the median as a mean, a sum that starts from +0.0, even for an odd count of nothing but -0.0.  The minimum
    # and the maximum keep the reference's sign where the anti-diagonal's zeros have one sign, and are compared with == elsewhere
    # (which of two equal zeros numpy's partition leaves in front is not determined); p50 is compared with == (see _same_summary).
    zeros = np.where(rng.random((n, w)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    mixed = np.where(rng.random((n, w)) < 0.6, zeros, base).astype(np.float32)
    onesign = np.where(rng.random((n, w)) < 0.6, np.float32(-0.0), base).astype(np.float32)
    for name, y in (("zeros", zeros), ("zeros among values", mixed), ("negative zeros among values", onesign)):
        free = _zero_sign_free(y)
        assert free.any() != (name == "negative zeros among values")
        ref = _oracle_unroll(y)
        assert (ref[0] == 0).sum() > n // 2
        assert not np.signbit(ref[0][ref[0] == 0]).any()
        worst = max(worst, _check_unroll(y, (name, w), sign_free=free, ref=ref))
    # infinities among finite values (medians only: np.percentile of such a diagonal is NaN through inf - inf)
    pick = rng.random((n, w))
    kinds = set()
    for name, (lo, hi) in (("a few infinities", (0.05, 0.95)), ("hardly a finite value", (0.48, 0.52))):
        inf = np.where(pick < lo, -np.inf, np.where(pick > hi, np.inf, base)).astype(np.float32)
        ref = _oracle_unroll(inf)
        kinds |= {k for k, f in (("+inf", np.isposinf), ("-inf", np.isneginf), ("nan", np.isnan), ("finite", np.isfinite)) if f(ref[0]).sum() >= 5}
        _check_unroll(inf, (name, w), summaries=(False,), fill=FILL, ref=ref)
    assert kinds == {"+inf", "-inf", "nan", "finite"}, kinds     # (nan: -inf and +inf as the two middle values, numpy's mean of them)
    # two middle values of 3e38: their mean overflows, as numpy's does
    big = np.where(rng.random((n, w)) < 0.2, base, np.float32(3e38)).astype(np.float32)
    ref = _oracle_unroll(big)
    assert np.isposinf(ref[0]).any() and (ref[0] == np.float32(3e38)).any()
    _check_unroll(big, ("3e38", w), summaries=(False,), ref=ref)
    print(f"\nscoring sweep unroll special values W={w}: worst quartile error / allowance {worst:.3f}")


def _nan_case(w, rng):
    n = w + 300
    y = rng.standard_normal((n, w)).astype(np.float32)
    y[0, 0] = np.nan                                        # the first timestep: an anti-diagonal of one value
    y[n - 1, w - 1] = np.nan                                # the last one
    y[200, w // 2] = np.nan                                 # interior anti-diagonal, outside the filter's 32-value sample at W >= 66
    y[260, min(5, w - 1)] = np.nan                          # inside the sample
    y[150, :] = np.nan                                      # a whole row: W consecutive timesteps
    hit = np.zeros(n + w - 1, dtype=bool)
    r, c = np.nonzero(np.isnan(y))
    hit[r + c] = True
    return y, hit


@pytest.mark.parametrize("w", [3, 64, 100, 129])
def test_unroll_nan_is_nan_as_numpy(w):
    """np.median, np.percentile, np.min and np.max of an anti-diagonal that holds a NaN are NaN: the median and all five summary values
    are NaN on exactly those timesteps, every other timestep keeps the reference's bits; the same through
    hypad_unroll_median_signals as one segment among three."""
    from hypad_amd import _C
    from hypad_amd.utils import anomaly_detection_utils as adu
    rng = np.random.default_rng(w + 3)
    y, hit = _nan_case(w, rng)
    ref = _oracle_unroll(y)
    assert np.array_equal(np.isnan(ref[0]), hit) and 0 < hit.sum() < len(hit) // 2
    _check_unroll(y, ("NaN", w), fill=FILL, ref=ref)
    single, _ = _unroll(_dev(y, torch.float32), False, FILL)
    others = [rng.standard_normal((k, w)).astype(np.float32) for k in (131, 70)]
    group = [others[0], y, others[1]]
    row_off = [int(v) for v in np.cumsum([0] + [len(g) for g in group])]
    t_off = adu.timestep_offsets(row_off, w)
    buf, med = _out(t_off[-1], torch.float32, FILL)
    _C.check(_C.lib.hypad_unroll_median_signals(_C.ptr(_dev(np.concatenate(group), torch.float32)), _C.ptr(med), 3, _C.int64s(row_off), w,
                                                _C.stream()), "unroll_median_signals")
    torch.cuda.synchronize()
    assert _intact(buf)
    med = med.cpu().numpy()
    for k, g in enumerate(group):
        want = single if k == 1 else sr.unroll_medians(g)
        _same_medians(med[t_off[k]: t_off[k + 1]], want, ("NaN, segment", k, w))


@pytest.mark.parametrize("w", [3, 5])
def test_unroll_second_iteration_of_the_tile_loop(w):
    """More than 8 192 tiles of 128 timesteps: the workgroups that take a second tile re-use the LDS tile behind the trailing barrier.
    Medians of all timesteps against the vectorised reference; with the summary (W = 5) the first and the last 2 000 timesteps
    against the oracle's loop."""
    n = 8192 * 128 + 300
    g = torch.Generator(device="cuda").manual_seed(w)
    d = torch.randn(n, w, device="cuda", generator=g)
    d[n // 2, 0] = d[n // 2 - 1, 1]                         # a tie far from both ends
    y = d.cpu().numpy()
    ref = sr.unroll_medians(y)
    med, _ = _unroll(d, False)
    _same_medians(med, ref, ("long", w, "medians only"))
    worst = 0.0
    if w == 5:
        med, summ = _unroll(d, True)
        _same_medians(med, ref, ("long", w, "summary"))
        k = 2000
        head, tail = _oracle_unroll(y[:k + w]), _oracle_unroll(y[-(k + w):])
        worst = max(_same_summary(summ[:k], med[:k], head[1][:k], ("long head", w)), _same_summary(summ[-k:], med[-k:], tail[1][-k:], ("long tail", w)))
        m64 = med.astype(np.float64)
        assert np.all(np.abs(summ[:, 2] - m64) <= 1e-6 * np.maximum(1.0, np.abs(m64))) and np.all(summ[:, 1:] >= summ[:, :-1])
    print(f"\nscoring sweep unroll long W={w}: worst quartile error / allowance {worst:.3f}")


# ------------------------------------------------------------------------------------------------ errors and rolling mean
def _err_call(name, y, yh, *extra, fill=NAN):
    """hypad_point_error / hypad_area_error / hypad_dtw_error of the device series (y float64, yh float32)."""
    from hypad_amd import _C
    t = y.numel()
    buf, out = _out(t, torch.float64, fill)
    _C.check(getattr(_C.lib, name)(_C.ptr(y), _C.ptr(yh), _C.ptr(out), t, *extra, _C.stream()), name)
    torch.cuda.synchronize()
    assert _intact(buf), (name, t, extra)
    return out.cpu().numpy()


def _rolling(x, w):
    from hypad_amd import _C
    t = x.numel()
    buf, out = _out(t, torch.float64, FILL)
    nbytes = _C.lib.hypad_rolling_workspace_bytes(t)
    ws = torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device="cuda")
    _C.check(_C.lib.hypad_rolling_mean(_C.ptr(x), None, _C.ptr(out), t, w, 0, ws.data_ptr(), nbytes, _C.stream()), "rolling_mean")
    torch.cuda.synchronize()
    assert _intact(buf), w
    return out.cpu().numpy()


def _pair(t, rng):
    y = rng.standard_normal(t)
    yh = (y + 0.1 * rng.standard_normal(t)).astype(np.float32)
    return y, yh


def _within(got, ref, tag, tol=1e-12):
    """|got - ref| <= tol max(1, max|ref|), NaN exactly where the reference has NaN; returns the worst error / allowance."""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), (tag, "NaN at", np.flatnonzero(np.isnan(got) != nan)[:8])
    if nan.all():
        return 0.0
    allow = tol * max(1.0, float(np.abs(ref[~nan]).max()))
    d = np.abs(got[~nan] - ref[~nan])
    assert d.max() <= allow, (tag, int(np.argmax(d)), float(d.max()), allow)
    return float(d.max()) / allow


@pytest.mark.parametrize("sw", [2, 3, 4, 5, 6, 8, 9, 10, 20, 21])
def test_dtw_error_every_instantiation(sw):
    """Window lengths 3, 5, 7, 9, 11, 21, each from both score windows that map to it.  y float64, y_hat float32 handed to the reference
    as the same values; zeros exactly where the reference has zeros.  (For a series shorter than LEN / 2 the reference returns LEN / 2
    zeros, more than the series has: its first T are compared.)"""
    from oracle import scoring as osc
    rng = np.random.default_rng(sw)
    length = (sw // 2) * 2 + 1
    worst = 0.0
    for t in sorted({1, length - 1, length, length + 1, length + 2, 255, 256, 257, 700}):
        y, yh = _pair(t, rng)
        got = _err_call("hypad_dtw_error", _dev(y, torch.float64), _dev(yh, torch.float32), sw)
        ref = (osc.dtw_error if t <= 64 else sr.dtw_error)(y, yh.astype(np.float64), sw)[:t]
        assert np.array_equal(got == 0, ref == 0), (sw, t, np.flatnonzero((got == 0) != (ref == 0))[:8])
        assert (ref != 0).sum() == max(t - length, 0)
        worst = max(worst, _within(got, ref, (sw, t)))
    # a series reconstructed exactly: all zeros, no NaN from the square root
    y = rng.standard_normal(300).astype(np.float32)
    got = _err_call("hypad_dtw_error", _dev(y, torch.float64), _dev(y, torch.float32), sw)
    assert np.all(got == 0) and not np.signbit(got).any()
    print(f"\nscoring sweep dtw score window {sw}: worst error / allowance {worst:.3f}")


@pytest.mark.parametrize("sw", [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 20, 21])
def test_area_error_every_window_and_short_series(sw):
    from oracle import scoring as osc
    rng = np.random.default_rng(100 + sw)
    worst = 0.0
    for t in sorted({1, 2, sw // 2 - 1, sw // 2, sw - 1, sw, sw + 1, 257} - {0, -1}):
        y, yh = _pair(t, rng)
        got = _err_call("hypad_area_error", _dev(y, torch.float64), _dev(yh, torch.float32), sw, fill=FILL)
        worst = max(worst, _within(got, osc.area_error(y, yh.astype(np.float64), sw), (sw, t)))
    print(f"\nscoring sweep area score window {sw}: worst error / allowance {worst:.3f}")


def test_grid_stride_loops_of_the_elementwise_kernels():
    """One series of 8 192 x 256 + 300 timesteps: the point, area, DTW and rolling-mean kernels each take a second pass of their
    grid-stride loop.  The point error is compared over all of it (one subtraction: exact), the others through the oracle on the first
    1 000, the last 1 000 and 1 000 timesteps around the first element of the second pass; the area error also over all of it against
    the vectorised reference."""
    from oracle import scoring as osc
    rng = np.random.default_rng(77)
    t = LONG_T
    y, yh = _pair(t, rng)
    h64 = yh.astype(np.float64)
    dy, dh = _dev(y, torch.float64), _dev(yh, torch.float32)
    ranges = ((0, 1000), (t - 1000, t), (8192 * 256 - 500, 8192 * 256 + 500))
    point = _err_call("hypad_point_error", dy, dh)
    assert np.array_equal(point, osc.point_error(y, h64))
    worst = {}
    area = _err_call("hypad_area_error", dy, dh, 10, fill=FILL)
    dtw = _err_call("hypad_dtw_error", dy, dh, 10)
    dpoint = _dev(point, torch.float64)
    roll = {w: _rolling(dpoint, w) for w in (10, 200)}
    ops = [("area", area, lambda a, b: osc.area_error(a, b, 10), (y, h64), 22), ("dtw", dtw, lambda a, b: osc.dtw_error(a, b, 10), (y, h64), 24),
           ("rolling 10", roll[10], lambda a: osc.rolling_mean_centered(a, 10), (point,), 22),
           ("rolling 200", roll[200], lambda a: osc.rolling_mean_centered(a, 200), (point,), 402)]
    for name, got, fn, series, halo in ops:
        worst[name] = max(_within(got[a:b], sr.oracle_slice(fn, series, halo, a, b), (name, a, b)) for a, b in ranges)
    worst["area, all"] = _within(area, sr.area_error(y, h64, 10), "area over the whole series")
    assert np.all(dtw[:5] == 0) and np.all(dtw[t - 6:] == 0) and np.all(dtw[5: t - 6] > 0)
    print("\nscoring sweep long series: worst error / allowance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------ KDE mode
def _kde(critic, w):
    from hypad_amd import _C
    c = _dev(critic, torch.float32)
    n = c.numel()
    buf, modes = _out(n + w - 1, torch.float64)
    _C.check(_C.lib.hypad_kde_mode(_C.ptr(c), _C.ptr(modes), n, w, _C.stream()), "kde_mode")
    torch.cuda.synchronize()
    assert _intact(buf), (n, w)
    return modes.cpu().numpy()


@pytest.mark.parametrize("w", [1, 2, 3, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256])
def test_kde_mode_at_the_edges_of_every_window_class(w):
    from oracle import scoring as osc
    from test_gpu_parity import _assert_same_modes_up_to_fp64_ties
    rng = np.random.default_rng(200 + w)
    n = w + 40
    for heavy in (False, True):
        cr = (rng.standard_t(2, n) if heavy else rng.standard_normal(n)).astype(np.float32)
        got = _kde(cr, w)
        ext = np.repeat(cr.astype(np.float64).reshape(-1, 1), w, axis=1)
        ref = np.array([osc.kde_mode(osc.antidiagonal(ext, i)) for i in range(n + w - 1)])
        _assert_same_modes_up_to_fp64_ties(cr, w, got, ref)
        print(f"\nscoring sweep kde W={w} {'t(2)' if heavy else 'normal'}: {int((got != ref).sum())} of {len(ref)} timesteps at an fp64 tie")


def test_kde_mode_past_one_grid_pass():
    """33 000 windows at W = 5: more timesteps than 8 192 workgroups x 4 waves."""
    from test_gpu_parity import _assert_same_modes_up_to_fp64_ties
    rng = np.random.default_rng(9)
    n, w = 33_000, 5
    assert n + w - 1 > 8192 * 4
    cr = rng.standard_normal(n).astype(np.float32)
    got, ref = _kde(cr, w), sr.kde_modes(cr, w)
    _assert_same_modes_up_to_fp64_ties(cr, w, got, ref)
    print(f"\nscoring sweep kde long: {int((got != ref).sum())} of {len(ref)} timesteps at an fp64 tie")


# ------------------------------------------------------------------------------------------------ row norms and combinations
def _norms(x, diff=None):
    from hypad_amd import _C
    rows, dim = x.shape
    buf, out = _out(rows, torch.float64)
    if diff is None:
        _C.check(_C.lib.hypad_row_norms(_C.ptr(x), _C.ptr(out), rows, dim, _C.stream()), "row_norms")
    else:
        _C.check(_C.lib.hypad_row_diff_norms(_C.ptr(x), _C.ptr(diff), _C.ptr(out), rows, dim, _C.stream()), "row_diff_norms")
    torch.cuda.synchronize()
    assert _intact(buf), (rows, dim)
    return out.cpu().numpy()


NORM_SHAPES = [(r, d) for d in (1, 63, 64, 65, 100, 256, 1000) for r in (1, 3, 4, 5)] + [(8192 * 4 + 5, 7)]


def test_row_norms_at_the_lane_and_grid_edges():
    """Under the sweep's rule (errgpu <= 8 err32 + 2e-6 against the fp64 norm, err32 that of np.linalg.norm on float32, which the kernel
    restates); hypad_row_diff_norms has the bits of hypad_row_norms on the fp32 difference."""
    rng = np.random.default_rng(31)
    ck = Checker("row norms")
    for rows, dim in NORM_SHAPES:
        a = (rng.standard_normal((rows, dim)) * 10.0 ** rng.integers(-2, 3, (rows, 1))).astype(np.float32)
        b = rng.standard_normal((rows, dim)).astype(np.float32)
        da, db = _dev(a, torch.float32), _dev(b, torch.float32)
        got = _norms(da)
        ck.cmp(f"norms {rows}x{dim}", got, np.linalg.norm(a.astype(np.float64), axis=1), np.linalg.norm(a, axis=1))
        diff = _norms(da, db)
        assert np.array_equal(_bits(diff), _bits(_norms((da - db).contiguous()))), (rows, dim)
        ck.cmp(f"diff norms {rows}x{dim}", diff, np.linalg.norm(a.astype(np.float64) - b.astype(np.float64), axis=1), np.linalg.norm(a - b, axis=1))
    print(f"\nscoring sweep row norms: worst errgpu / allowance {ck.worst:.3f}")
    ck.done()


COMB_READS = {"sum": "cr", "mult": "cr", "uncertainty": "cru", "critic": "c", "critic_uncertainty": "cu", "sum_uncertainty": "cru", "rec": "r",
              "rec_uncertainty": "ru", "eucl_mult": "cr", "eucl_sum": "cr"}


def _comb_ref(mode, c, r, u):
    """(reference, sum of |terms|) of one combination."""
    from oracle import scoring as osc
    if mode.startswith("eucl_"):
        ref = osc.combine_euclidean(mode[5:], c, r)
        terms = np.abs(c * r) if mode == "eucl_mult" else np.abs(0.5 * (c - 1)) + np.abs(0.5 * (r - 1))
        return ref, terms
    ref = osc.combine_scores(mode, c, r, u.reshape(-1, 1))
    terms = {"sum": lambda: np.abs(0.2 * c) + np.abs(0.8 * r), "mult": lambda: np.abs(c * r), "uncertainty": lambda: np.abs(c * r * u),
             "critic": lambda: np.zeros_like(c), "critic_uncertainty": lambda: np.abs(c * u),
             "sum_uncertainty": lambda: np.abs(0.5 * c * u) + np.abs(0.5 * r * u), "rec": lambda: np.zeros_like(c),
             "rec_uncertainty": lambda: np.abs(r * u)}[mode]()
    return ref, terms


@pytest.mark.parametrize("n", [1, 255, 256, 257, 8192 * 256 + 3])
def test_combine_scores_every_mode(n):
    """All ten modes, the operands a mode does not read passed as NULL, within 4 x 2^-52 x (sum of |terms|) of the reference: the device
    may contract a product and a sum into one fused multiply-add where numpy rounds twice.  Where the reference overflows or is NaN
    (1e150 x 1e150, inf - inf) the device has the same value."""
    from hypad_amd import _C
    rng = np.random.default_rng(n)
    special = np.array([0.0, -1.0, 1e150, 1e-150, -1e150, -2.5e-150, 1.0, 3.0])

    def values(nonneg):
        v = rng.standard_normal(n) * 3.0
        k = rng.random(n) < 0.3
        v[k] = special[rng.integers(0, len(special), int(k.sum()))]
        return np.abs(v) if nonneg else v
    c, r, u = values(False), values(False), values(True)      # (u: row norms, never negative)
    dev = {"c": _dev(c, torch.float64), "r": _dev(r, torch.float64), "u": _dev(u, torch.float64)}
    worst = 0.0
    for mode, reads in COMB_READS.items():
        buf, out = _out(n, torch.float64, FILL)
        args = [_C.ptr(dev[k]) if k in reads else None for k in "cru"]
        _C.check(_C.lib.hypad_combine_scores(_C.COMB[mode], *args, _C.ptr(out), n, _C.stream()), mode)
        torch.cuda.synchronize()
        assert _intact(buf), mode
        got = out.cpu().numpy()
        ref, terms = _quiet(_comb_ref, mode, c, r, u)
        odd = ~np.isfinite(ref)
        assert np.array_equal(got[odd], ref[odd], equal_nan=True), (mode, n)
        allow = 4 * 2.0 ** -52 * terms[~odd]
        d = np.abs(got[~odd] - ref[~odd])
        assert np.all(d <= allow), (mode, n, int(np.argmax(d - allow)), float((d - allow).max()))
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(allow > 0, d / allow, 0.0), initial=0.0)))
    print(f"\nscoring sweep combine n={n}: worst error / allowance {worst:.3f}")
