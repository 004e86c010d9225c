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
"""
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
