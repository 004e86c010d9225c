"""tests/scoring_ref.py against oracle/scoring.py (no GPU): the vectorised restatements the GPU sweep uses at sizes the oracle's loops
cannot reach are the oracle's functions, the slice helper returns the oracle's values of the whole series, the filter model is the
decision written in csrc/unroll_median_body.inc, and every input family of the sweep reaches the branch it is there for."""
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
