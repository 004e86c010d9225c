"""tests/scoring_ref.py against oracle/scoring.py (no GPU): the vectorised restatements the GPU sweep uses at sizes the oracle's loops
cannot reach are the oracle's functions, the slice helper returns the oracle's values of the whole series, the filter model is the
decision written in csrc/unroll_median_body.inc, and every input family of the sweep reaches the branch it is there for.

The second half does the same for the statistics sweep (tests/test_gpu_scoring_statistics.py): the exact rolling mean, z-score and
trimmed critic z-score are the oracle's, the O(T) form of the rolling mean is the fsum form, the key model orders doubles as numbers,
every quantile input takes the route it is named for (decided, listed, exactly 4 096 candidates, fall-back), the tied inputs have
their quartiles on tied samples, and the NaN layouts of the rolling mean empty the chunks and meet and miss min_periods as named."""
import warnings

import numpy as np
import pytest

import scoring_ref as sr
from oracle import scoring as osc


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize("n,w", [(1, 1), (7, 1), (1, 5), (2, 7), (4, 5), (5, 5), (6, 5), (40, 2), (64, 3), (130, 100), (300, 64), (37, 256), (400, 129)])
def test_vectorised_medians_are_the_oracles_bits(n, w):
    rng = np.random.default_rng(n * 1000 + w)
    y = rng.standard_normal((n, w)).astype(np.float32)
    y[rng.integers(0, n), rng.integers(0, w)] = y[0, 0]
    ref, _ = osc.unroll_predictions(y, False)
    got = sr.unroll_medians(y)
    assert got.dtype == ref.dtype == np.float32 and np.array_equal(_bits(got), _bits(ref))
    z = (np.round(y * 10) / 10).astype(np.float32)          # ties, and means of two middle values
    assert np.array_equal(_bits(sr.unroll_medians(z)), _bits(osc.unroll_predictions(z, False)[0]))


def test_vectorised_medians_overflow_and_nan_like_numpy():
    y = np.random.default_rng(0).standard_normal((40, 4)).astype(np.float32)
    y[10:30, :] = np.float32(3e38)
    y[33, 2] = np.nan
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        ref, got = osc.unroll_predictions(y, False)[0], sr.unroll_medians(y)
    assert np.isinf(ref).any() and np.isnan(ref).sum() == 1
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)])


@pytest.mark.parametrize("w", [2, 3, 4, 5, 10, 11, 20, 21])
def test_vectorised_area_and_dtw_errors_are_the_oracles(w):
    rng = np.random.default_rng(w)
    for t in (1, 2, w // 2, w - 1, w, w + 1, 2 * w + 3, 97):
        if t < 1:
            continue
        y = rng.standard_normal(t)
        h = (y + 0.1 * rng.standard_normal(t)).astype(np.float32).astype(np.float64)
        ref, got = osc.area_error(y, h, w), sr.area_error(y, h, w)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (w, t)
        assert np.allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True), (w, t)
        ref, got = osc.dtw_error(y, h, w), sr.dtw_error(y, h, w, chunk=16)
        assert got.shape == ref.shape and np.array_equal(got == 0, ref == 0), (w, t)
        assert np.abs(got - ref).max() <= 1e-12, (w, t)


def test_vectorised_area_error_takes_the_ends_of_a_long_series_from_the_oracle():
    rng = np.random.default_rng(5)
    y = rng.standard_normal(400)
    h = y + 0.1 * rng.standard_normal(400)
    for w in (7, 10):
        ref, got = osc.area_error(y, h, w), sr.area_error(y, h, w)
        assert np.allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True) and np.array_equal(np.isnan(got), np.isnan(ref))


@pytest.mark.parametrize("n,w", [(1, 1), (9, 1), (1, 4), (3, 5), (5, 5), (30, 2), (60, 7), (300, 5), (90, 64)])
def test_vectorised_kde_modes_pick_the_oracles_sample(n, w):
    rng = np.random.default_rng(10 * n + w)
    for c in (rng.standard_normal(n), rng.standard_t(2, n)):
        c = c.astype(np.float32)
        ext = np.repeat(c.astype(np.float64).reshape(-1, 1), w, axis=1)
        ref = np.array([osc.kde_mode(osc.antidiagonal(ext, i)) for i in range(n + w - 1)])
        assert np.array_equal(sr.kde_modes(c, w), ref), (n, w)
    ones = np.ones(n, np.float32)                           # singular covariance: the median
    ext = np.repeat(ones.astype(np.float64).reshape(-1, 1), w, axis=1)
    assert np.array_equal(sr.kde_modes(ones, w), np.array([osc.kde_mode(osc.antidiagonal(ext, i)) for i in range(n + w - 1)]))


def test_oracle_slice_returns_the_values_of_the_whole_series():
    rng = np.random.default_rng(2)
    t = 900
    y = rng.standard_normal(t)
    h = (y + 0.1 * rng.standard_normal(t)).astype(np.float32).astype(np.float64)
    ops = [("point", osc.point_error, (y, h), 0), ("area 10", lambda a, b: osc.area_error(a, b, 10), (y, h), 22),
           ("area 7", lambda a, b: osc.area_error(a, b, 7), (y, h), 16), ("dtw 10", lambda a, b: osc.dtw_error(a, b, 10), (y, h), 22),
           ("dtw 3", lambda a, b: osc.dtw_error(a, b, 3), (y, h), 8), ("roll 10", lambda a: osc.rolling_mean_centered(a, 10), (np.abs(y - h),), 22),
           ("roll 200", lambda a: osc.rolling_mean_centered(a, 200), (np.abs(y - h),), 402)]
    for name, fn, series, halo in ops:
        whole = np.asarray(fn(*series))
        for a, b in ((0, 60), (0, t), (430, 470), (t - 60, t), (300, 301)):
            part = sr.oracle_slice(fn, series, halo, a, b)
            assert part.shape == (b - a,) and np.array_equal(np.isnan(part), np.isnan(whole[a:b])), (name, a, b)
            if name.startswith("roll"):     # pandas adds and removes one value per step: a window's sum carries the rounding of where the pass began
                assert np.allclose(part, whole[a:b], rtol=0, atol=1e-14, equal_nan=True), (name, a, b)
            else:
                assert np.array_equal(part, whole[a:b], equal_nan=True), (name, a, b)


def _kernel_text_filter(v):
    """The filter's decision transcribed line by line from csrc/unroll_median_body.inc (scalar loops, fp32 compares)."""
    v = [np.float32(x) for x in v]
    cnt = len(v)
    less = [sum(1 for k in range(32) if v[k] < v[i]) for i in range(32)]
    plo, phi = np.float32(-np.inf), np.float32(np.inf)
    for i in range(32):
        if less[i] <= 10:
            plo = max(plo, v[i])
        if less[i] >= 21:
            phi = min(phi, v[i])
    c_lt = sum(1 for x in v if x < plo)
    c_le = sum(1 for x in v if x <= phi)
    cand = [x for x in v if plo <= x <= phi]
    nc, m1, m2 = c_le - c_lt, (cnt - 1) >> 1, cnt >> 1
    if not (c_lt <= m1 and m2 < c_le and nc <= 64 and nc > 0):
        return "pivot_miss" if not (c_lt <= m1 and m2 < c_le and nc > 0) else "many"
    assert len(cand) == nc
    rk = [sum(1 for q in cand if q < c) for c in cand]
    return "hit" if sum(rk) == nc * (nc - 1) // 2 else "cand_ties"


def test_filter_model_is_the_kernels_decision():
    rng = np.random.default_rng(9)
    seen = set()
    for name in sr.FAMILIES:
        for w in (64, 100, 129):
            y = sr.family(name, w, n=w + 40)
            for t in rng.integers(63, w + 40, 12):
                v = sr.tile_order(y, int(t))
                if len(v) >= sr.FILTER_MIN:
                    b = sr.filter_branch(v)
                    assert b == _kernel_text_filter(v), (name, w, int(t))
                    seen.add(b)
    assert seen == set(sr.BRANCHES)
    # tile order: element k of timestep t is y_hat[t - j0 - k, j0 + k]
    y = sr.family("gaussian", 70, n=90)
    for t, j0 in ((75, 0), (100, 11)):
        v = sr.tile_order(y, t)
        assert all(v[k] == y[t - j0 - k, j0 + k] for k in range(len(v))) and len(v) == min(t + 1, 70) - j0


@pytest.mark.parametrize("w", sr.FILTER_WINDOWS)
def test_every_family_reaches_its_branch(w):
    """The coverage condition of the GPU sweep's filter test (a property of the inputs, not of the kernel): at n = W + 300 every family
    sends at least 20 timesteps down the path it is there for.  'many' needs more than 64 candidates: it cannot occur at window 64, and
    the narrow-tail family, whose candidates are at most the 33 values outside the sample plus the sample's middle, cannot reach it at
    window 65 either."""
    for name, (_, branch, exempt) in sr.FAMILIES.items():
        if w in exempt:
            continue
        counts = sr.branch_counts(sr.family(name, w))
        assert counts[branch] >= sr.MIN_BRANCH_TIMESTEPS, (name, w, counts)
    assert sr.branch_counts(sr.family("constant", 64))["many"] == 0


# ------------------------------------------------------------------------------------------------ the statistics sweep's references
@pytest.mark.parametrize("w", sr.ROLL_WS)
def test_exact_rolling_mean_is_the_oracles(w):
    """NaN exactly where pandas has NaN, values within 1e-12 max(1, |ref|); with the fused subtrahend too."""
    for t in sr.roll_short_ts(w) + [1400]:
        for layout in ("none", "scattered", "min periods"):
            if not sr.layout_fits(t, w, 0, layout):
                continue
            x = sr.roll_input(t, w, 0, layout)
            ref, got = osc.rolling_mean_centered(x, w), sr.rolling_mean_exact(x, w)
            assert np.array_equal(np.isnan(got), np.isnan(ref)), (w, t, layout)
            ok = ~np.isnan(ref)
            assert np.all(np.abs(got[ok] - ref[ok]) <= 1e-12 * np.maximum(1.0, np.abs(ref[ok]))), (w, t, layout)
    x = sr.roll_input(300, w, 0, "none")
    sub = (x + 0.1).astype(np.float32)
    sub[::17] = np.nan
    ref = osc.rolling_mean_centered(np.abs(x - sub.astype(np.float64)), w)
    got = sr.rolling_mean_exact(x, w, sub)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.allclose(got, ref, rtol=0, atol=1e-12, equal_nan=True)


@pytest.mark.parametrize("w", [1, 2, 33, 257, 1250])
def test_prefix_sum_form_of_the_exact_rolling_mean_is_the_fsum_form(w):
    assert np.finfo(sr.LD).nmant >= 63                       # (the references' extended precision)
    for t, layout in ((1, "none"), (w + 1, "none"), (700, "scattered"), (2000, "min periods"), (1300, "run 600")):
        x = sr.roll_input(t, w, 5, layout) * 10.0 ** np.random.default_rng(t).integers(-30, 30, t)
        a, b = sr.rolling_mean_exact(x, w, extended=True), sr.rolling_mean_exact_long(x, w)
        assert np.array_equal(np.isnan(a), np.isnan(b)), (w, t, layout)
        ok = ~np.isnan(a)
        assert np.all(np.abs(a[ok] - b[ok]) <= 2.0 ** -60 * np.abs(b[ok])), (w, t, layout)
        d = sr.rolling_mean_exact(x, w)
        assert np.all(np.abs(d[ok] - b[ok]) <= 2.0 ** -52 * np.abs(b[ok]))


@pytest.mark.parametrize("t", [2, 7, 257, 1025, 5000])
def test_exact_zscores_are_the_oracles(t):
    """On well-conditioned input (the oracle is fp64 numpy / scipy): within 1e-12; all NaN where the oracle is all NaN."""
    rng = np.random.default_rng(t)
    x = 3.0 + rng.standard_normal(t)
    assert np.abs(sr.zscore_exact(x).astype(np.float64) - osc.zscore_clip(x)).max() <= 1e-12
    v = sr.tied_input(4 * t + 1)
    lo, hi, nlo, nhi = sr.ties_at_quartiles(v)
    got = sr.critic_zscore_exact(v, lo, hi).astype(np.float64)
    assert np.abs(got - osc.compute_critic_score(v, 1)).max() <= 1e-12
    mean, sd = sr.exact_moments(x)
    assert abs(float(mean) - x.mean()) <= 1e-14 and abs(float(sd) - x.std()) <= 1e-14
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for family in ("constant", "nan in the last slice", "one +inf"):
            y = sr.stat_input(family, t)
            assert np.isnan(osc.zscore_clip(y)).all() and np.isnan(sr.zscore_exact(y)).all(), family
        for family in ("constant", "nan in the last slice", "one +inf"):
            y = sr.stat_input(family, t)
            lo, hi = np.quantile(y, 0.25), np.quantile(y, 0.75)
            assert np.isnan(osc.compute_critic_score(y, 1)).all() and np.isnan(sr.critic_zscore_exact(y, lo, hi)).all(), family


def test_statistics_allowance_counts_and_slices():
    """stat_slices restates stat_blocks and the slice arithmetic of the partials kernels: no slice is empty, together they are the
    series; the counts of the allowance at the sizes of the sweep; numpy's own fp64 result lies inside the allowance."""
    for t in list(range(1, 3000)) + list(sr.STAT_TS) + [262144 + 1023, 262144 * 3 + 1]:
        sl = sr.stat_slices(t)
        assert len(sl) == sr.stat_blocks(t) and sl[0][0] == 0 and sl[-1][1] == t
        assert all(e > b for b, e in sl) and all(sl[i][1] == sl[i + 1][0] for i in range(len(sl) - 1)), t
    assert [sr.stat_blocks(t) for t in (1023, 1024, 1025, 262143, 262144, 262145)] == [1, 1, 2, 256, 256, 256]
    assert sr.stat_counts(1024) == (13, 70, 80) and sr.stat_counts(262145)[0] == 5 + 9 and sr.stat_counts(2097155)[0] == 33 + 9
    assert [e - b for b, e in sr.stat_slices(1025)] == [513, 512]                # an uneven last slice
    assert {e - b for b, e in sr.stat_slices(2097155)} == {8193, 7940} and [e - b for b, e in sr.stat_slices(2049)] == [683] * 3      # (g = 3: no power of two)
    for family in ("normal", "mean 1e6", "ramp"):
        x = sr.stat_input(family, 5000)
        mean, sd = sr.exact_moments(x)
        ref = sr.zscore_exact(x)
        assert np.all(np.abs(osc.zscore_clip(x) - ref) <= sr.zscore_allowance(x, ref, mean, sd)), family


def test_key_model_orders_doubles_as_numbers():
    v = np.array([-np.inf, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.0 + 2.0 ** -52, 2.0, 1e300, np.inf])
    k = sr.qs_keys(v)
    assert np.all(k[1:] > k[:-1])
    band = sr.band_values(5000, np.random.default_rng(0))
    assert len(np.unique(band)) == 5000 and len(np.unique(sr.qs_keys(band) >> np.uint64(31))) == 1
    assert sr.quantile_ranks(5, 0.25) == (1, 2) and sr.quantile_ranks(5, 1.0) == (4, 4) and sr.quantile_ranks(1, 0.3) == (0, 0)


def test_every_quantile_input_takes_its_route():
    """What lets the GPU test claim the edges of the candidate list: at m = 4 095 and 4 096 the quartile and median ranks are 'listed'
    with exactly m candidates, at 4 097 and 8 192 they fall back; q = (0, 1) reads a list of two and a single key; the mixed calls
    have one quantile on each route; the long band family falls back with every value a candidate; the long continuous families are
    listed."""
    for m in sr.BAND_SIZES:
        x = sr.band_input(m)
        assert len(x) == m + 3000
        want = (m, "listed" if m <= sr.QS_CAND else "fallback")
        for q in sr.BAND_QS[:2]:
            assert sr.band_count(x, q) == [want] * (2 * len(q)), (m, q)
        assert sr.band_count(x, (0.0, 1.0)) == [(2, "listed")] * 2 + [(1, "decided")] * 2
    x = sr.band_input(4097, 1)
    fb, li, de = (4097, "fallback"), (2, "listed"), (1, "decided")
    assert [sr.band_count(x, q) for q in sr.MIXED_QS] == [[fb, fb, li, li], [li, li, fb, fb], [de, de, fb, fb]]
    for n in sr.LONG_NS:
        assert n > 1024 * 1024
        assert sr.band_count(sr.long_input("band", n), (0.25, 0.75)) == [(n, "fallback")] * 4
        for family in ("normal", "fp32 origin"):
            got = sr.band_count(sr.long_input(family, n), (0.25, 0.75))
            assert all(r in ("listed", "decided") for _, r in got), (family, n, got)


@pytest.mark.parametrize("n", sr.TIED_NS)
def test_tied_inputs_have_their_quartiles_on_tied_samples(n):
    x = sr.tied_input(n)
    lo, hi, nlo, nhi = sr.ties_at_quartiles(x)
    assert ((n - 1) * 0.25).is_integer() and ((n - 1) * 0.75).is_integer()
    assert nlo >= sr.MIN_TIES and nhi >= sr.MIN_TIES, (nlo, nhi)
    # an exclusive end would move the trimmed mean by far more than the allowance
    inc, exc = x[(x >= lo) & (x <= hi)].mean(), x[(x >= lo) & (x < hi)].mean()
    mean, sd = sr.exact_moments(x)
    allow = sr.zscore_allowance(x, sr.critic_zscore_exact(x, lo, hi), inc, sd, trimmed=True).max()
    assert abs(inc - exc) / float(sd) > 1e6 * allow


def test_rolling_layouts_have_the_edges_they_are_named_for():
    for w, origin in sr.ROLL_LONG_PAIRS:
        for t in sr.ROLL_LONG_TS:
            assert sr.empty_chunks(sr.roll_input(t, w, origin, "run 16 aligned"), origin, 16) == 1
            assert sr.empty_chunks(sr.roll_input(t, w, origin, "run 16 off by one"), origin, 16) == 0
            x = sr.roll_input(t, w, origin, "run 256 aligned")
            assert sr.empty_chunks(x, origin, 256) == 1 and sr.empty_chunks(x, origin, 16) == 16
            assert sr.empty_chunks(sr.roll_input(t, w, origin, "run 600"), origin, 256) >= 1
            c = sr.window_counts(sr.roll_input(t, w, origin, "min periods"), w)
            assert (c == w // 2).any() and (c == w // 2 - 1).any(), (w, origin, t)
    for w in sr.ROLL_WS:
        if w >= 4:
            assert sr.layout_fits(600, w, 0, "min periods") == (w <= 257)      # (the short GPU test has this layout up to w = 257; 1 250 in the long one)
            if w <= 257:
                c = sr.window_counts(sr.roll_input(600, w, 0, "min periods"), w)
                assert (c == w // 2).any() and (c == w // 2 - 1).any(), w
            assert sr.window_counts(sr.roll_input(w // 2 - 1, w, 0, "none"), w).max() == w // 2 - 1      # a series too short for any window
            assert sr.window_counts(sr.roll_input(w // 2, w, 0, "none"), w).max() == w // 2
    assert {o % 16 for o in sr.ROLL_ORIGINS} >= {0, 1, 15, 5} and {o % 256 for o in sr.ROLL_ORIGINS} >= {0, 1, 255}
    assert {o for _, o in sr.ROLL_LONG_PAIRS} | {1} == set(sr.ROLL_ORIGINS) and {w for w, _ in sr.ROLL_LONG_PAIRS} == {33, 257, 1250}
