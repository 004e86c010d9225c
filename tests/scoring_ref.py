"""References of the scoring sweep (tests/test_gpu_scoring_sweep.py on the GPU, tests/test_scoring_reference.py on the CPU).

The reference of every scoring kernel is ``oracle/scoring.py``.  Its Python loops take tens of seconds at the sizes where the kernels'
grid-stride loops run a second time (more than 8 192 workgroups), so this module restates four of its functions in vectorised form --
the interior timesteps as one strided matrix reduced along its rows, the 2 (W - 1) edge timesteps through the oracle's own loop.  The
restatements are no second opinion: tests/test_scoring_reference.py pins each of them to the oracle function on small shapes (medians
bit for bit, area and DTW errors within 1e-12, the KDE mode by its arg-max).

``oracle_slice`` gives the oracle's own values of a local operation (point, area, DTW error, rolling mean) on a range of a long series
without running the oracle over all of it.

``filter_branch`` is a NumPy model of the decision the two-pivot filter of ``csrc/unroll_median_body.inc`` takes for one anti-diagonal;
``FAMILIES`` are the inputs that steer it into each of its outcomes, and ``branch_counts`` is what the host test checks before the GPU
test may claim that it has run every outcome.  The model says which path a timestep takes, never what the median is.

The second half serves the statistics sweep (tests/test_gpu_scoring_statistics.py): exact references of the centred rolling mean, the
z-score and the trimmed critic z-score, the allowances counted from the kernel text, a NumPy model of the quantile selection's key
and of the route a rank takes (``band_count``), and the inputs of that sweep with the properties they are built for.
"""
import math

import numpy as np

from oracle import scoring as osc


# ------------------------------------------------------------------------------------------------ vectorised restatements
def _interior_diagonals(y_hat):
    """(n - W + 1, W) view: row i holds the anti-diagonal of timestep t = W - 1 + i, in DESCENDING column order
    (element k is y_hat[t - (W - 1) + k, W - 1 - k])."""
    n, w = y_hat.shape
    flat = np.ascontiguousarray(y_hat).reshape(-1)
    item = flat.strides[0]
    return np.lib.stride_tricks.as_strided(flat[w - 1:], shape=(n - w + 1, w), strides=(w * item, (w - 1) * item), writeable=False)


def unroll_medians(y_hat):
    """``oracle.scoring.unroll_predictions(y_hat, False)[0]``: np.median of every anti-diagonal, in y_hat's dtype."""
    y_hat = np.asarray(y_hat)
    n, w = y_hat.shape
    t = n + w - 1
    med = np.empty(t, dtype=y_hat.dtype)
    lo, hi = (w - 1, n) if n >= w else (t, t)              # interior timesteps [lo, hi): all W columns present
    for i in list(range(0, min(lo, t))) + list(range(max(hi, 0), t)):
        med[i] = np.median(osc.antidiagonal(y_hat, i))
    if hi > lo:
        with np.errstate(all="ignore"):
            med[lo:hi] = np.median(_interior_diagonals(y_hat), axis=1)
    return med


def _windows(x, w, chunk=1 << 18):
    """Consecutive (rows, w) sliding-window blocks of the 1-D array x, at most `chunk` rows each: (first window index, block)."""
    v = np.lib.stride_tricks.sliding_window_view(x, w)
    for a in range(0, v.shape[0], chunk):
        yield a, v[a:a + chunk]


def _rolling_trapezoid(x, w):
    """pandas ``rolling(w, center=True, min_periods=w // 2).apply(np.trapezoid)`` of the 1-D fp64 array x."""
    x = np.asarray(x, dtype=np.float64)
    t = len(x)
    out = np.full(t, np.nan)
    off = (w - 1) // 2                                      # pandas' centred window of i: [i + off - w + 1, i + off]
    first, last = w - 1 - off, t - 1 - off                  # interior timesteps [first, last]: the whole window inside the series
    if last >= first:
        for a, blk in _windows(x, w):
            out[first + a: first + a + blk.shape[0]] = np.trapezoid(blk, axis=1)
    edge = [i for i in range(t) if i < first or i > last]
    if edge:
        ref = osc._rolling_apply_centered(x, w, w // 2, np.trapezoid) if t <= 4 * w + 8 else None
        for i in edge:
            if ref is not None:
                out[i] = ref[i]
            else:                                           # a long series: the oracle on the end that holds timestep i
                a, b = (0, 3 * w) if i < first else (t - 3 * w, t)
                out[i] = osc._rolling_apply_centered(x[a:b], w, w // 2, np.trapezoid)[i - a]
    return out


def area_error(y, y_hat, score_window=10):
    """``oracle.scoring.area_error``."""
    return np.abs(_rolling_trapezoid(y, score_window) - _rolling_trapezoid(y_hat, score_window))


def dtw_error(y, y_hat, score_window=10, chunk=1 << 14):
    """``oracle.scoring.dtw_error``: the recurrence of ``dtw_classic`` on all windows of a chunk at once, cell by cell in the oracle's order
    (cumulative sums along the first row and column, then ``c + min(up, left, diagonal)``).  Like the oracle (and the reference it
    restates) it returns ``half`` zeros for a series shorter than ``half``: more values than the series has."""
    length = (score_window // 2) * 2 + 1
    half = length // 2
    y, y_hat = np.asarray(y, dtype=np.float64), np.asarray(y_hat, dtype=np.float64)
    t = len(y)
    nsim = max(t - length, 0)
    out = np.zeros(max(t, half))
    if nsim == 0:
        return out
    yp, hp = np.pad(y, (half, half)), np.pad(y_hat, (half, half))
    for (a, xa), (_, xb) in zip(_windows(yp, length, chunk), _windows(hp, length, chunk)):
        xa, xb = xa[: max(nsim - a, 0)], xb[: max(nsim - a, 0)]
        if not len(xa):
            break
        c = (xa[:, :, None] - xb[:, None, :]) ** 2
        d = np.empty_like(c)
        d[:, 0, :] = np.cumsum(c[:, 0, :], axis=1)
        d[:, :, 0] = np.cumsum(c[:, :, 0], axis=1)
        for i in range(1, length):
            for j in range(1, length):
                d[:, i, j] = c[:, i, j] + np.minimum(np.minimum(d[:, i - 1, j], d[:, i, j - 1]), d[:, i - 1, j - 1])
        out[half + a: half + a + len(xa)] = np.sqrt(d[:, -1, -1])
    return out


def kde_modes(critic, window):
    """``oracle.scoring.kde_mode`` of every anti-diagonal of the critic values repeated along the window (final_critic_scores): the
    sample with the largest Scott-bandwidth Gaussian density, the first one in anti-diagonal order, the median where the variance is
    zero or there is one sample."""
    c = np.asarray(critic, dtype=np.float64).reshape(-1)
    n, w = len(c), int(window)
    t = n + w - 1
    out = np.empty(t)
    ext = None
    lo, hi = (w - 1, n) if n >= w else (t, t)
    edge = list(range(0, min(lo, t))) + list(range(max(hi, 0), t))
    if edge:
        # the oracle's own loop on the two ends (only the rows an edge diagonal can touch are materialised)
        k = min(n, 2 * w)
        head = np.repeat(c[:k].reshape(-1, 1), w, axis=1)
        tail = np.repeat(c[n - k:].reshape(-1, 1), w, axis=1)
        for i in edge:
            if n <= 2 * w:
                ext = np.repeat(c.reshape(-1, 1), w, axis=1) if ext is None else ext
                out[i] = osc.kde_mode(osc.antidiagonal(ext, i))
            elif i < lo:
                out[i] = osc.kde_mode(osc.antidiagonal(head, i))
            else:
                out[i] = osc.kde_mode(osc.antidiagonal(tail, i - (n - k)))
    if hi > lo:
        if w == 1:
            out[lo:hi] = c
            return out
        factor2 = float(w) ** (-0.4)                        # Scott's factor n^(-1/5), squared
        for a, blk in _windows(c, w, max(1, (1 << 22) // (w * w))):      # (a chunk's pair matrix: 32 MB)
            v = blk[:, ::-1]                                # sample j of timestep t is critic[t - j]
            cov = np.var(v, axis=1, ddof=1) * factor2
            ok = cov > 0
            with np.errstate(all="ignore"):
                d = v[:, :, None] - v[:, None, :]
                dens = np.exp(-(d * d) / (2.0 * cov[:, None, None])).sum(axis=2)
            pick = np.where(ok, np.argmax(np.where(ok[:, None], dens, 0.0), axis=1), 0)
            res = v[np.arange(len(v)), pick]
            if not ok.all():
                res = np.where(ok, res, np.median(v, axis=1))
            out[lo + a: lo + a + len(v)] = res
    return out


# ------------------------------------------------------------------------------------------------ the oracle on a range
def oracle_slice(fn, series, halo, a, b):
    """``fn(*series)[a:b]`` -- the oracle function fn of the full 1-D series -- computed on [a - halo, b + halo) only.  ``halo`` is how
    far the operation looks to either side plus the width of its own end effects, so a cut that is no end of the series does not
    reach [a, b); where the range touches an end of the series the slice has that end too and the values come out as on the whole."""
    t = len(series[0])
    lo, hi = max(0, a - halo), min(t, b + halo)
    return np.asarray(fn(*[np.asarray(s)[lo:hi] for s in series]))[a - lo: b - lo]


# ------------------------------------------------------------------------------------------------ the filter's decision
FILTER_MIN = 64          # the filter looks at anti-diagonals of at least 64 values (medians only)
BRANCHES = ("hit", "pivot_miss", "many", "cand_ties")


def tile_order(y_hat, t):
    """The anti-diagonal of timestep t as the kernel's LDS row holds it: v[k] = y_hat[t - j0 - k, j0 + k]."""
    return osc.antidiagonal(y_hat, t)


def filter_branch(v):
    """Which way the two-pivot filter goes for the anti-diagonal ``v`` (>= 64 float32 values in tile order):
    'hit'        the middle lies between the pivots, at most 64 candidates, all different: the candidates alone are ranked;
    'pivot_miss' the middle position(s) do not lie between the pivots;
    'many'       they do, but more than 64 values lie between the pivots;
    'cand_ties'  they do, at most 64 candidates, two of them equal;
    the last three take the full rank count."""
    v = np.asarray(v, dtype=np.float32)
    cnt = len(v)
    assert cnt >= FILTER_MIN
    s = v[:32]
    less = (s[None, :] < s[:, None]).sum(axis=1)            # ranks inside the sample
    lo, hi = s[less <= 10], s[less >= 21]
    plo = lo.max() if len(lo) else np.float32(-np.inf)      # largest sample with at most 10 below it
    phi = hi.min() if len(hi) else np.float32(np.inf)       # smallest sample with at least 21 below it
    c_lt, c_le = int((v < plo).sum()), int((v <= phi).sum())
    nc = c_le - c_lt
    m1, m2 = (cnt - 1) >> 1, cnt >> 1
    if not (c_lt <= m1 and m2 < c_le and nc > 0):
        return "pivot_miss"
    if nc > 64:
        return "many"
    cand = v[(v >= plo) & (v <= phi)]
    return "cand_ties" if len(np.unique(cand)) < len(cand) else "hit"


def _gaussian(n, w, seed):
    return np.random.default_rng(seed).standard_normal((n, w)).astype(np.float32)


def _two_decimals(n, w, seed):
    return (np.round(_gaussian(n, w, seed) * 100) / 100).astype(np.float32)


def _column_ramp(n, w, seed):
    # every value of column j below every value of column j + 1: the 32-value sample is the 32 smallest of its anti-diagonal
    return (np.arange(w, dtype=np.float32)[None, :] + 0.25 * np.random.default_rng(seed).random((n, w), dtype=np.float32)).astype(np.float32)


def _constant(n, w, seed):
    return np.full((n, w), np.float32(0.625 + seed % 3), dtype=np.float32)


def _narrow_tail(n, w, seed):
    # a wide sample (columns 0 .. 31) and a narrow rest: nearly every value lies between the pivots
    y = _gaussian(n, w, seed)
    y[:, 32:] *= np.float32(0.01)
    return y


# name -> (generator(n, W, seed), the branch the family is there for, the windows at which it cannot be reached)
FAMILIES = {
    "gaussian": (_gaussian, "hit", ()),
    "two_decimals": (_two_decimals, "cand_ties", ()),
    "column_ramp": (_column_ramp, "pivot_miss", ()),
    "constant": (_constant, "many", (64,)),                 # 64 equal values are 64 candidates: 'cand_ties'
    "narrow_tail": (_narrow_tail, "many", (64, 65)),        # at most 33 values outside the sample
}
FILTER_WINDOWS = (64, 65, 100, 128, 129, 200, 256)
MIN_BRANCH_TIMESTEPS = 20


def family(name, w, n=None):
    """The (n, W) float32 input of a family (n = W + 300 unless given; seeded by the window)."""
    return FAMILIES[name][0](w + 300 if n is None else n, w, 1000 + w)


def branch_counts(y_hat):
    """{branch: timesteps} over the anti-diagonals of at least 64 values."""
    n, w = y_hat.shape
    out = dict.fromkeys(BRANCHES, 0)
    for t in range(n + w - 1):
        v = tile_order(y_hat, t)
        if len(v) >= FILTER_MIN:
            out[filter_branch(v)] += 1
    return out


# ------------------------------------------------------------------------------------------------ exact statistics
# References of the statistics sweep (tests/test_gpu_scoring_statistics.py): the centred rolling mean, the z-score and the trimmed
# critic z-score with every sum taken exactly (math.fsum) and the remaining operations in np.longdouble (a 64-bit significand: the
# reference's own error is below 2^-60 of the value, 1 % of the smallest allowance it is compared under, one rounding at 2^-53).
# tests/test_scoring_reference.py pins them to oracle/scoring.py.
LD = np.longdouble
U = 2.0 ** -53                                              # unit roundoff of fp64: one rounded operation errs by at most U |result|


def _fsum2(values):
    """The exact sum of a list of floats as (s, r): s the correctly rounded sum, r the rounded remainder (s + r errs by 2^-106)."""
    s = math.fsum(values)
    return s, (math.fsum(values + [-s]) if math.isfinite(s) else 0.0)


def centred_window(i, w, t):
    """pandas' rolling(w, center=True) window of timestep i in a series of t: the inclusive range [lo, hi]."""
    off = (w - 1) // 2
    return max(0, i + off - w + 1), min(t - 1, i + off)


def rolling_values(x, sub=None):
    """The series hypad_rolling_mean smooths: x, or the point-wise error |x - sub| (sub float32, widened) -- one fp64 subtraction."""
    x = np.asarray(x, dtype=np.float64)
    return x if sub is None else np.abs(x - np.asarray(sub, dtype=np.float32).astype(np.float64))


def rolling_mean_exact(x, w, sub=None, extended=False):
    """pandas ``rolling(w, center=True, min_periods=w // 2).mean()`` of the finite-or-NaN series: for every timestep math.fsum of its
    window's non-NaN values and one division; NaN where fewer than w // 2 (or none) are valid.  extended=True: np.longdouble, the
    sum's remainder included."""
    v = rolling_values(x, sub)
    t = len(v)
    ok = v == v
    out = np.full(t, np.nan, dtype=LD if extended else np.float64)
    for i in range(t):
        lo, hi = centred_window(i, w, t)
        seg = v[lo:hi + 1][ok[lo:hi + 1]].tolist()
        cnt = len(seg)
        if cnt > 0 and cnt >= w // 2:
            if extended:
                s, r = _fsum2(seg)
                out[i] = (LD(s) + LD(r)) / cnt
            else:
                out[i] = math.fsum(seg) / cnt
    return out


def rolling_mean_exact_long(x, w, sub=None):
    """``rolling_mean_exact(x, w, sub, extended=True)`` in O(T): the values as integers times one power of two, exact prefix sums in
    Python integers, every window's mean as an exact fraction rounded once (tests/test_scoring_reference.py pins it to the fsum form)."""
    v = rolling_values(x, sub)
    t = len(v)
    ok = v == v
    m, ex = np.frexp(np.where(ok, v, 0.0))
    mi = (m * 2.0 ** 53).astype(np.int64).tolist()          # exact: |m| < 1 with at most 53 bits
    ex = (ex.astype(np.int64) - 53).tolist()
    e0 = min([e for a, e in zip(mi, ex) if a] or [0])
    pre = [0] * (t + 1)
    for i in range(t):
        pre[i + 1] = pre[i] + ((mi[i] << (ex[i] - e0)) if mi[i] else 0)
    cnts = np.concatenate([[0], np.cumsum(ok)]).tolist()
    d, r = np.full(t, np.nan), np.zeros(t)
    for i in range(t):
        lo, hi = centred_window(i, w, t)
        cnt = cnts[hi + 1] - cnts[lo]
        if cnt > 0 and cnt >= w // 2:
            num = pre[hi + 1] - pre[lo]                      # the mean is num 2^e0 / cnt = a / b
            a, b = (num << e0, cnt) if e0 >= 0 else (num, cnt << -e0)
            d[i] = a / b                                     # (Python's integer division rounds the exact quotient once)
            dn, dd = d[i].as_integer_ratio()
            r[i] = (a * dd - dn * b) / (b * dd)
    return d.astype(LD) + r.astype(LD)


def window_counts(x, w, sub=None):
    """Valid (non-NaN) values in every timestep's centred window."""
    v = rolling_values(x, sub)
    c = np.concatenate([[0], np.cumsum(v == v)])
    t = len(v)
    return np.array([c[hi + 1] - c[lo] for lo, hi in (centred_window(i, w, t) for i in range(t))])


def empty_chunks(x, origin, size):
    """How many aligned chunks of `size` absolute positions (the series starts at position `origin`) lie inside the series and hold
    nothing but NaN: what empties a 16- or 256-chunk sum of the rolling mean's workspace."""
    x = np.asarray(x)
    first = -origin % size
    return sum(1 for a in range(first, len(x) - size + 1, size) if np.isnan(x[a:a + size]).all())


def _exact_mean(x):
    s, r = _fsum2(np.asarray(x, dtype=np.float64).tolist())
    return (LD(s) + LD(r)) / len(x)


def exact_moments(x):
    """(mean, population standard deviation) of the finite fp64 vector x in np.longdouble: the mean from the exact sum, the squared
    deviations and their (pairwise, all-positive) sum in longdouble.  NaN, NaN for a series that is not finite."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all():
        return LD(np.nan), LD(np.nan)
    mean = _exact_mean(x)
    d = x.astype(LD) - mean
    return mean, np.sqrt(np.sum(d * d) / len(x))


def zscore_exact(x, moments=None):
    """``oracle.scoring.zscore_clip``: max((x - mean) / sd, 0) + 1 in np.longdouble, NaN everywhere for a constant series (0 / 0) and for one that holds a NaN or an infinity (inf - inf in the deviations)."""
    x = np.asarray(x, dtype=np.float64)
    if not np.isfinite(x).all() or (x == x[0]).all():
        return np.full(len(x), np.nan, dtype=LD)
    mean, sd = moments or exact_moments(x)
    return np.maximum((x.astype(LD) - mean) / sd, 0) + 1


def critic_zscore_exact(x, lo, hi, moments=None, with_mean=False):
    """``oracle.scoring.compute_critic_score`` without its rolling mean: |x - mean of the values inside [lo, hi]| / sd + 1, both ends
    inclusive, in np.longdouble; NaN everywhere where the series is constant or not finite or no value lies inside the range."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        inside = (x >= lo) & (x <= hi)
    if not np.isfinite(x).all() or (x == x[0]).all() or not inside.any():
        out = np.full(len(x), np.nan, dtype=LD)
        return (out, LD(np.nan)) if with_mean else out
    _, sd = moments or exact_moments(x)
    mean = _exact_mean(x[inside])
    out = np.abs(x.astype(LD) - mean) / sd + 1
    return (out, mean) if with_mean else out


# ---- allowances of the statistics kernels, from their text (csrc/scoring.hip).  U = 2^-53; first-order in U throughout.
ROLL_DIRECT_MAX = 32


def rolling_additions(w):
    """Additions on the longest path from a value to its window's sum in hypad_rolling_mean.
    Direct form (w <= 32): the window is summed left to right, w - 1 additions (the first lands on 0.0 exactly).
    Chunked form: the running sum takes at most 15 single values in front of the first 16-aligned position and 15 behind the last, at
    most 15 16-chunk sums in front of the first 256-aligned position and 15 behind the last, and w // 256 256-chunk sums -- one addition
    each; a value that arrives inside a chunk sum has been through at most 15 additions inside its 16-chunk and 15 more where the
    256-chunk adds its 16 16-chunk sums."""
    return w - 1 if w <= ROLL_DIRECT_MAX else (15 + 15) + (15 + 15) + w // 256 + 15 + 15


def rolling_allowance(x, w, sub=None):
    """(A + 1) U sum|v| / cnt per timestep: A additions of at most U (partial sum) <= U sum|v| each, one division."""
    return (rolling_additions(w) + 1) * U * rolling_mean_exact_long(np.abs(rolling_values(x, sub)), w).astype(np.float64)


STAT_G = 256


def stat_blocks(t):
    return min(max((t + 1023) // 1024, 1), STAT_G)


def stat_slices(t):
    """[(begin, end)] of the slices the statistics kernels cut a series of t values into (stat_blocks(t) of ceil(t / blocks))."""
    g = stat_blocks(t)
    ln = (t + g - 1) // g
    return [(b * ln, min(b * ln + ln, t)) for b in range(g)]


def stat_counts(t):
    """(ksum, kmean, km2): rounded operations on the longest path of the two-level statistics of t values.
    ksum   one block sum: ceil(len / 256) strided additions per thread, six butterfly steps, three additions of the four wave sums.
    kmean  the mean: a block sum and its division by n, then eight levels of stat_merge, each of four rounded operations (the difference
           of the two means, b.n / r.n, their product, the sum) on quantities of at most 2 max|x|, 1, 2 max|x| and max|x|: at most
           7 U max|x| a level.
    km2    M2, relative (all its terms are positive): a deviation (two uses in the square), the square, a block sum; per merge level the
           two additions, d twice, two products, a.n b.n and its division by r.n: eight."""
    ln = max(e - b for b, e in stat_slices(t))
    ksum = -(-ln // 256) + 6 + 3
    return ksum, ksum + 1 + 8 * 7, ksum + 3 + 8 * 8


def zscore_allowance(x, out, mean, sd, trimmed=False):
    """What hypad_zscore_clip (trimmed=False: out = max(z, 0) + 1, z = (x - mean) / sd) or hypad_critic_zscore (trimmed=True:
    out = |x - mean| / sd + 1, mean the trimmed mean) may be off by, per element, against the exact `out`, `mean` and `sd`.
        |error of the mean|  <= km U max|x|         km = kmean (trimmed: ksum + 8 merge additions + the division, of in-range values)
        numerator x - mean   <= that + U |x - mean|
        relative error of sd <= (km2 / 2 + 2) U + kmean U max|x| / sd
              half of M2's, the division by n and the root; the last term is what the slice means' own errors do to the merged M2:
              d (sum n_s (m_s - M)^2) = 2 sum n_s (m_s - M) dm_s <= 2 n sd max|dm_s| (Cauchy-Schwarz), relative to M2 = n sd^2, halved
        the quotient         one more U, the + 1 one more U |out|
    so |error| <= (km max|x| + |x - mean|) U / sd + v ((km2 / 2 + 3) + kmean max|x| / sd) U + U |out|, v = |x - mean| / sd."""
    x = np.asarray(x, dtype=np.float64)
    ksum, kmean, km2 = stat_counts(len(x))
    km = ksum + 9 if trimmed else kmean
    amax, sd, dev = float(np.abs(x).max()), float(sd), np.abs(x - float(mean))
    v = dev / sd
    return ((km * amax + dev) / sd + v * ((km2 / 2 + 3) + kmean * amax / sd) + np.abs(np.asarray(out, dtype=np.float64))) * U


# ------------------------------------------------------------------------------------------------ the quantile routes
QS_CAND = 4096
ROUTES = ("decided", "listed", "fallback")


def qs_keys(x):
    """csrc/scoring.hip qs_key: the 64-bit key whose unsigned order is the numeric order of the doubles (-0.0 below +0.0)."""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0x8000000000000000))


def quantile_ranks(n, q):
    """The two order statistics np.quantile (method 'linear') interpolates for q: floor((n - 1) q) and the next, both n - 1 at the end."""
    pos = (n - 1) * float(q)
    if pos >= n - 1:
        return n - 1, n - 1
    lo = max(int(math.floor(pos)), 0)
    return lo, min(lo + 1, n - 1)


def band_count(x, q):
    """For every rank the quantiles q select (two per quantile, in order): (how many values share the 33-bit key prefix of the value of
    that rank, the route the selection takes for it): 'decided' when all of them are one key (no list is read), 'listed' for up to
    QS_CAND = 4 096 of them (the candidate list is ranked), 'fallback' beyond (the last three radix levels run over the input)."""
    k = np.sort(qs_keys(x))
    pre = k >> np.uint64(31)
    out = []
    for qq in np.atleast_1d(q):
        for r in quantile_ranks(len(k), qq):
            a, b = np.searchsorted(pre, pre[r], "left"), np.searchsorted(pre, pre[r], "right")
            out.append((int(b - a), "decided" if k[a] == k[b - 1] else "listed" if b - a <= QS_CAND else "fallback"))
    return out


# ------------------------------------------------------------------------------------------------ inputs of the statistics sweep
# (built here so that tests/test_scoring_reference.py can assert on the CPU that each has the edge the GPU test names it for)
def band_values(m, rng):
    """m different values 1 + j 2^-52, j < 2^31: one 33-bit key prefix (sign, exponent, 21 mantissa bits), the low 31 bits differ."""
    j = rng.choice(1 << 31, size=m, replace=False) if m <= 1 << 16 else rng.integers(0, 1 << 31, m)
    return 1.0 + j.astype(np.float64) * 2.0 ** -52


def band_input(m, seed=0, below=1500, above=1500):
    """A band of m values with one key prefix, `below` values under 0.9 and `above` over 2.0, shuffled.  The values below come as pairs
    of neighbouring doubles (two keys under one prefix: a candidate list of two), the values above alone (one key: decided)."""
    rng = np.random.default_rng(1000 * seed + m)
    low = rng.uniform(0.1, 0.9, below // 2)
    x = np.concatenate([band_values(m, rng), low, np.nextafter(low, 1.0), rng.uniform(2.0, 9.0, above)])
    rng.shuffle(x)
    return x


BAND_SIZES = (4095, 4096, 4097, 8192)
BAND_QS = ((0.25, 0.75), (0.5,), (0.0, 1.0))
MIXED_QS = ((0.5, 0.01), (0.01, 0.5), (0.99, 0.5))         # one quantile inside the band of 4 097, the other among the scattered values
LONG_NS = (1048576 + 1025, 2 * 1048576 + 3)                 # past one pass of 1 024 workgroups x 1 024 values, and past two


def long_input(family, n):
    rng = np.random.default_rng(n % 1000 + len(family))
    if family == "normal":
        return rng.standard_normal(n)
    if family == "fp32 origin":
        return rng.standard_normal(n).astype(np.float32).astype(np.float64)
    assert family == "band"
    return band_values(n, rng)


def tied_input(n, seed=0):
    """fp32 values rounded to two decimals, widened: with n = 1 (mod 4) the 25 % and 75 % quantiles are samples, and tied ones."""
    assert n % 4 == 1
    v = np.random.default_rng(seed + n).standard_normal(n)
    return (np.round(v * 100) / 100).astype(np.float32).astype(np.float64)


TIED_NS = (16385, 262145, 2097153)
MIN_TIES = 20


def ties_at_quartiles(x):
    """(lo, hi, values equal to lo, values equal to hi) for the quartiles np.quantile gives."""
    lo, hi = np.quantile(x, 0.25), np.quantile(x, 0.75)
    return lo, hi, int((x == lo).sum()), int((x == hi).sum())


STAT_TS = (1, 2, 255, 256, 257, 1023, 1024, 1025, 2049, 262143, 262144, 262145, 2097155)
STAT_FAMILIES = ("normal", "mean 1e6", "mean 1e-3 spread 1e3", "constant", "nan in the last slice", "one +inf", "ramp")


def stat_input(family, t):
    rng = np.random.default_rng(t + 7 * STAT_FAMILIES.index(family))
    x = rng.standard_normal(t)
    if family == "mean 1e6":
        x += 1e6
    elif family == "mean 1e-3 spread 1e3":
        x = 1e-3 + 1e3 * x
    elif family == "constant":
        x[:] = 2.5                                           # every partial sum exact: 0 / 0.  (A constant whose sums round, 0.1, has no
        #                                                      reference: scipy calls a series constant when std <= eps |mean| of its own fp64
        #                                                      mean, which 1 025 values of 0.1 miss and 7 meet.)
    elif family == "nan in the last slice":
        b, e = stat_slices(t)[-1]
        x[(b + e) // 2] = np.nan
    elif family == "one +inf":
        x[t // 3] = np.inf
    elif family == "ramp":
        x = np.arange(t) / 7.0 + 0.01 * x
    return x


ROLL_WS = (1, 2, 3, 31, 32, 33, 34, 255, 256, 257, 511, 513, 1250)
ROLL_ORIGINS = (0, 1, 15, 16, 17, 255, 256, 257, 4095, (1 << 31) + 5)
ROLL_LONG_TS = (4095, 4096, 4097, 6000)
# (w, origin) at T = 4 095 .. 6 000: every origin class, w = 33, 257 and 1 250 each at an aligned origin, one off by one, and a large one
ROLL_LONG_PAIRS = ((33, 0), (33, 15), (33, 17), (33, 256), (257, 0), (257, 1), (257, 16), (257, 255), (257, 4095), (1250, 0), (1250, 257),
                   (1250, (1 << 31) + 5))
ROLL_LAYOUTS = ("none", "scattered", "run 16 aligned", "run 16 off by one", "run 256 aligned", "run 600", "min periods")


def roll_short_ts(w):
    return sorted({1, w // 2 - 1, w // 2, w - 1, w, w + 1, 600} - {0, -1})


def _roll_places(t, w, origin):
    return 16 + -origin % 16, 256 + -origin % 256, w - w // 2 + 1


def layout_fits(t, w, origin, layout):
    """Whether a series of t values has room for the NaN layout (roll_input refuses one that has not)."""
    at16, at256, run = _roll_places(t, w, origin)
    return {"none": True, "scattered": True, "run 16 aligned": at16 + 16 <= t, "run 16 off by one": at16 + 17 <= t,
            "run 256 aligned": at256 + 256 <= t, "run 600": t >= 1000, "min periods": t >= w + run + 4}[layout]


def roll_input(t, w, origin, layout, seed=0):
    """A positive-and-negative series of t values with the NaN layout `layout`; runs are placed on ABSOLUTE chunk boundaries (position =
    origin + index)."""
    assert layout_fits(t, w, origin, layout), (t, w, origin, layout)
    rng = np.random.default_rng(seed + 31 * t + w)
    x = rng.standard_normal(t) + 0.5
    at16, at256, run = _roll_places(t, w, origin)
    if layout == "scattered":
        x[rng.integers(0, t, max(1, t // 100))] = np.nan
    elif layout == "run 16 aligned":
        x[at16: at16 + 16] = np.nan
    elif layout == "run 16 off by one":
        x[at16 + 1: at16 + 17] = np.nan
    elif layout == "run 256 aligned":
        x[at256: at256 + 256] = np.nan
    elif layout == "run 600":
        x[333: 933] = np.nan
    elif layout == "min periods":
        # a run one longer than ceil(w / 2): a window that holds all of it has w // 2 - 1 valid values, one that misses one of its values
        # has exactly w // 2
        a = (t - run) // 2
        x[a: a + run] = np.nan
    return x
