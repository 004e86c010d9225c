"""Window scoring on the GPU (reference: utils/anomaly_detection_utils.py).

Same function names and argument meaning as the reference for the numerics on the hot path
(SURVEY.md §8a rows S1-S6); inputs may be NumPy arrays (as the reference passes) or device tensors, results
come back as NumPy arrays like the reference's.  Interval extraction and the overlap-segment metrics
 are host-side NumPy in ``hypad_amd.utils.intervals`` and re-exported here under the reference's
names.  The reference's cached artefacts are kept under their names and formats -- ``critic_scores.pickle``,
``point.pickle`` / ``area.pickle`` / ``dtw.pickle`` (:229-235, :470-550), ``anomalies.csv`` (:94-95) and the results table
``./results/<params.filename>`` (:115-126) -- whenever a ``path`` is given; plotting is not part of this module.
"""
import ctypes
import math
import os
import pickle

import numpy as np
import torch

from .. import _C
from ..hyperspace import gmath
from .intervals import (_find_sequences, _find_threshold, _fixed_threshold, _merge_sequences, _overlap, _prune_anomalies,  # noqa: F401
                        casas_anomalies, compute_metrics, contextual_confusion_matrix, find_anomalies)


COMBINATIONS = ("sum", "mult", "uncertainty", "critic", "critic_uncertainty", "sum_uncertainty", "rec", "rec_uncertainty")    # combine_scores (:336-362)
EUCLIDEAN_MODES = {"mult": "eucl_mult", "sum": "eucl_sum", "rec": "rec", "critic": "critic"}         # score_anomalies' ``comb`` (:553-570) -> _C.COMB
# find_anomalies' settings of the two detectors (:89-95 and :183-187; fixed_threshold=True in both)
UNIVARIATE_INTERVALS = dict(window_size_portion=0.33, window_step_size_portion=0.1)
MULTIVARIATE_INTERVALS = dict(window_size_portion=0.2, window_step_size_portion=0.1, anomaly_padding=200)


def uses_critic(combination):
    """Whether a combination of COMBINATIONS reads the critic scores (:70-73, :166-169)."""
    return combination not in ("rec", "rec_uncertainty")


def _euclidean_mode(comb):
    mode = EUCLIDEAN_MODES.get(comb)
    if mode is None:
        raise ValueError('Unknown combination specified {}, use "mult", "sum", or "rec" instead.'.format(comb))
    return mode


def _dev():
    return torch.device("cuda")


def _f32(a):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(_dev(), torch.float32).contiguous()


def _f64(a):
    t = a if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a))
    return t.to(_dev(), torch.float64).contiguous()


def unroll_true(y):
    """First sample of every window plus the tail of the last (:908-910).  y: (N, S) or (N, S, 1)."""
    if isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.float32 and y.is_contiguous():
        y = y.reshape(y.shape[0], -1)               # the matrix the forward read: take the n + S - 1 values straight from it
        n, w = y.shape
        out = torch.empty(n + w - 1, device=y.device, dtype=torch.float64)
        _C.check(_C.lib.hypad_unroll_true_f32(_C.ptr(y), w, _C.ptr(out), n, w, _C.stream()), "unroll_true_f32")
        return out
    y = _f64(y)
    y = y.reshape(y.shape[0], -1)
    n, w = y.shape
    out = torch.empty(n + w - 1, device=y.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_unroll_true(_C.ptr(y), _C.ptr(out), n, w, _C.stream()), "unroll_true")
    return out


def unroll_predictions(y_hat, with_summary=True):
    """Per-timestep median (float32) and [min, p25, p50, p75, max] over the anti-diagonals (:918-935)."""
    y_hat = _f32(y_hat)
    n, w = y_hat.shape
    t = n + w - 1
    med = torch.empty(t, device=y_hat.device, dtype=torch.float32)
    summ = torch.empty(t, 5, device=y_hat.device, dtype=torch.float64) if with_summary else None
    _C.check(_C.lib.hypad_unroll_median(_C.ptr(y_hat), _C.ptr(med), _C.ptr(summ), n, w, _C.stream()), "unroll_median")
    return med, summ


def _point_wise_error(y, y_hat):
    y, y_hat = _f64(y), _f32(y_hat)
    out = torch.empty_like(y)
    _C.check(_C.lib.hypad_point_error(_C.ptr(y), _C.ptr(y_hat), _C.ptr(out), y.numel(), _C.stream()), "point_error")
    return out


def _area_error(y, y_hat, score_window=10):
    y, y_hat = _f64(y), _f32(y_hat)
    out = torch.empty_like(y)
    _C.check(_C.lib.hypad_area_error(_C.ptr(y), _C.ptr(y_hat), _C.ptr(out), y.numel(), score_window, _C.stream()), "area_error")
    return out


def _dtw_error(y, y_hat, score_window=10):
    y, y_hat = _f64(y), _f32(y_hat)
    out = torch.empty_like(y)
    _C.check(_C.lib.hypad_dtw_error(_C.ptr(y), _C.ptr(y_hat), _C.ptr(out), y.numel(), score_window, _C.stream()), "dtw_error")
    return out


_SCRATCH = {}


def _scratch(device, nbytes, tag):
    """A scratch buffer for the library calls' workspaces, per device AND stream (grown, never shrunk; stream-ordered like everything
    here -- two branches of a pass that run beside each other on two streams, `concurrently`, must not share one)."""
    key = (str(device), tag, _C.stream().value if torch.device(device).type == "cuda" else None)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _SCRATCH[key] = torch.empty(max(int(nbytes), 64), dtype=torch.uint8, device=device)
    return buf


_SIDE_STREAMS = {}


def concurrently(fn_main, fn_side):
    """``fn_main()`` on the current stream and ``fn_side()`` on a side stream BESIDE it: both start behind everything queued so far,
    whatever is queued afterwards starts behind both.  Returns (fn_main(), fn_side()).  What it is for: the critic smoothing of a
    scoring pass is one chip-filling kernel (the KDE modes, 0.26 ms per 125 000 windows) plus ~10 launch-sized ones, the
    reconstruction numerics are ~12 launch-sized kernels (0.17 ms): independent of each other, both read only the forward's outputs,
    and beside each other the small launches disappear under the large one.  Capturable (the fork and the join become graph edges)."""
    dev = torch.cuda.current_device()
    main = torch.cuda.current_stream()
    side = _SIDE_STREAMS.get((dev, main.cuda_stream))
    if side is None:                                   # (one whose work really runs beside main's: streams can share a hardware queue)
        from .. import streams
        side = _SIDE_STREAMS[(dev, main.cuda_stream)] = streams.beside([main], dev)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        b = fn_side()
    a = fn_main()
    main.wait_stream(side)
    return a, b


def rolling_mean(x, window, origin=0, minus=None):
    """pandas ``rolling(window, center=True, min_periods=window // 2).mean()`` (:953-961, :325-330).  ``window == 0`` -- the
    reference's ``math.trunc(n * 0.01)`` for fewer than 100 windows -- gives all-NaN, as pandas does.  ``minus``: smooth the
    point-wise error ``|x - minus|`` (:761-777) without materialising it.  ``origin``: position of ``x[0]`` in the whole series
    when ``x`` is a slice of it (the sums are taken in an order fixed by absolute positions: a slice gives the whole's bits)."""
    x = _f64(x)
    if int(window) == 0:
        return torch.full_like(x, float("nan"))
    out = torch.empty_like(x)
    sub = None if minus is None else _f32(minus)
    nbytes = _C.lib.hypad_rolling_workspace_bytes(x.numel())
    ws = _scratch(x.device, nbytes, "roll")
    _C.check(_C.lib.hypad_rolling_mean(_C.ptr(x), _C.ptr(sub), _C.ptr(out), x.numel(), int(window), int(origin), ws.data_ptr(), nbytes,
                                       _C.stream()), "rolling_mean")
    return out


def zscore_clip(x):
    """stats.zscore(x) -> clip(min=0) + 1  (:523-524)."""
    x = _f64(x)
    out = torch.empty_like(x)
    ws = _scratch(x.device, _C.STATS_WORKSPACE_BYTES, "stats")
    _C.check(_C.lib.hypad_zscore_clip(_C.ptr(x), _C.ptr(out), x.numel(), ws.data_ptr(), _C.STATS_WORKSPACE_BYTES, _C.stream()), "zscore_clip")
    return out


def reconstruction_errors(y, y_hat, step_size=1, score_window=10, smoothing_window=0.01, smooth=True, rec_error_type="point",
                          with_summary=True):
    """:866-962.  Returns (errors, predictions_vs) as NumPy arrays like the reference."""
    if step_size != 1:
        raise NotImplementedError("step_size != 1 (the reference's callers always use 1)")
    n = len(y)
    if isinstance(smoothing_window, float):
        smoothing_window = min(math.trunc(n * smoothing_window), 200)
    true = unroll_true(y)
    pred, summ = unroll_predictions(y_hat, with_summary)
    kind = rec_error_type.lower()
    if kind == "point" and smooth and smoothing_window:
        err = rolling_mean(true, smoothing_window, minus=pred)         # |true - pred| smoothed in one pass
        smooth = False
    elif kind == "point":
        err = _point_wise_error(true, pred)
    elif kind == "area":
        err = _area_error(true, pred, score_window)
    elif kind == "dtw":
        err = _dtw_error(true, pred, score_window)
    else:
        raise ValueError(rec_error_type)
    if smooth:
        err = rolling_mean(err, smoothing_window)
    pvs = summ.cpu().numpy().reshape(-1, 1, 5) if summ is not None else np.empty((0, 1, 5))
    return err.cpu().numpy(), pvs


def hyperbolic_rec_scores(recons_signal, true_signal, signal_shape):
    """Row-wise Poincare distance between real windows on the ball and reconstructions (:54-66)."""
    true_data = _f32(recons_signal).reshape(-1, signal_shape)
    pred_data = _f32(true_signal).reshape(-1, signal_shape)
    return gmath.poincare_rowdist(pred_data, true_data)


def row_norms(x):
    x = _f32(x)
    out = torch.empty(x.shape[0], device=x.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_row_norms(_C.ptr(x), _C.ptr(out), x.shape[0], x.shape[1], _C.stream()), "row_norms")
    return out


def row_diff_norms(a, b):
    """np.linalg.norm(a - b, axis=1) of two fp32 matrices, the difference formed in fp32 on the device (:157, :160-161): the bits of
    row_norms on the fp32 matrix a - b."""
    a, b = _f32(a), _f32(b)
    if a.shape != b.shape or a.dim() != 2:
        raise ValueError(f"row_diff_norms: shapes {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty(a.shape[0], device=a.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_row_diff_norms(_C.ptr(a), _C.ptr(b), _C.ptr(out), a.shape[0], a.shape[1], _C.stream()), "row_diff_norms")
    return out


def combine_scores(combination, critic_scores=[], rec_scores=[], recons_signal=[], norms=None, as_tensor=False):
    """:336-362.  ``norms``: the row norms of ``recons_signal`` when the caller already has them (sharded scoring);
    ``as_tensor``: leave the result on the device instead of returning NumPy."""
    if combination not in COMBINATIONS:
        raise ValueError(combination)
    c = _f64(critic_scores) if len(critic_scores) else None
    r = _f64(rec_scores) if len(rec_scores) else None
    n = (r if r is not None else c).numel()
    u = None
    if "uncertainty" in combination:
        u = (_f64(norms) if norms is not None else row_norms(recons_signal))[:n].contiguous()
    if c is not None:
        c = c[:n].contiguous()
    out = torch.empty(n, device=_dev(), dtype=torch.float64)
    _C.check(_C.lib.hypad_combine_scores(_C.COMB[combination], _C.ptr(c), _C.ptr(r), _C.ptr(u), _C.ptr(out), n, _C.stream()), "combine")
    return out if as_tensor else out.cpu().numpy()


def combine_euclidean(comb, critic_scores, rec_scores, as_tensor=False):
    """Tail of score_anomalies (:553-570), lambda_rec = 0.5."""
    mode = _euclidean_mode(comb)
    c, r = _f64(critic_scores), _f64(rec_scores)
    out = torch.empty_like(r)
    _C.check(_C.lib.hypad_combine_scores(_C.COMB[mode], _C.ptr(c), _C.ptr(r), None, _C.ptr(out), r.numel(), _C.stream()), "combine")
    return out if as_tensor else out.cpu().numpy()


def quantiles(x, q):
    """``np.quantile(x, q)`` (method "linear") of a device vector for one or two ``q``: exact order statistics by radix
    selection (hypad_quantiles), the result stays on the device -- (len(q),) float64."""
    c = _f64(x).reshape(-1)
    q = [float(v) for v in np.atleast_1d(q)]
    qa = (ctypes.c_double * len(q))(*q)
    out = torch.empty(len(q), dtype=torch.float64, device=c.device)
    nbytes = _C.lib.hypad_quantile_workspace_bytes()
    ws = _scratch(c.device, nbytes, "quantiles")
    _C.check(_C.lib.hypad_quantiles(_C.ptr(c), c.numel(), qa, len(q), _C.ptr(out), ws.data_ptr(), nbytes, _C.stream()), "quantiles")
    return out


def _compute_critic_score(critics, smooth_window):
    """:307-333 -- quantile-trimmed mean, |z| + 1, centred rolling mean.  All on the device: the two quantiles by radix
    selection (no sort), one reduction kernel, one elementwise kernel, the rolling mean; nothing passes through the host."""
    c = _f64(critics)
    out = torch.empty_like(c)
    nbytes = _C.lib.hypad_critic_score_workspace_bytes()
    ws = _scratch(c.device, nbytes, "critic_score")
    _C.check(_C.lib.hypad_critic_score(_C.ptr(c), _C.ptr(out), c.numel(), ws.data_ptr(), nbytes, _C.stream()), "critic_score")
    return rolling_mean(out, smooth_window)


def kde_modes(critic_score, window):
    """Per un-rolled timestep, the KDE mode of the covering windows' critic values (:374-400)."""
    c = _f32(critic_score).reshape(-1)
    n = c.numel()
    modes = torch.empty(n + window - 1, device=c.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_kde_mode(_C.ptr(c), _C.ptr(modes), n, int(window), _C.stream()), "kde_mode")
    return modes


def final_critic_scores(critic_score, true_signal):
    """:365-404."""
    n, w = true_signal.shape[0], true_signal.shape[1]
    return _compute_critic_score(kde_modes(critic_score, w), math.trunc(n * 0.01)).cpu().numpy()


def _load_pickle(file):
    with open(file, "rb") as handle:
        return pickle.load(handle)


def _dump_pickle(obj, file):
    with open(file, "wb") as handle:
        pickle.dump(obj, handle, protocol=pickle.HIGHEST_PROTOCOL)


def compute_critic_scores(rec_scores, critic_score, true_signal, params, path):
    """:225-238 -- the smoothed KDE critic scores of the hyperbolic / multivariate branches, cached as
    ``path + "critic_scores.pickle"`` (read back only when ``params.load`` is set, always re-written otherwise)."""
    file = (path or "") + "critic_scores.pickle"
    if path and getattr(params, "load", False) and os.path.exists(file):
        critic_scores = np.asarray(_load_pickle(file))
    else:
        ts = np.asarray(true_signal)
        critic_scores = final_critic_scores(critic_score, ts.reshape(len(ts), -1))
        if path:
            _dump_pickle(critic_scores, file)
    return critic_scores[: len(rec_scores)]


def score_anomalies(y, y_hat, critic, index=None, score_window=10, critic_smooth_window=None, error_smooth_window=None,
                    smooth=True, rec_error_type="point", comb="mult", lambda_rec=0.5, path=None, samples_num="0", with_true=True):
    """:407-576.  Returns (final_scores, true_index, true, predictions) (``with_true=False``: ``true`` = [], see below).  With a ``path`` the reference's caches are kept:
    ``critic_scores.pickle`` is read if present (else computed and written); the z-scored reconstruction scores of all three
    error types are written as ``point.pickle`` / ``area.pickle`` / ``dtw.pickle`` when missing, and the requested one is read
    back if it was there already (``predictions`` is then empty, as in the reference)."""
    if lambda_rec != 0.5:
        raise NotImplementedError("lambda_rec != 0.5")
    n = y.shape[0]
    critic_smooth_window = critic_smooth_window or math.trunc(n * 0.01)
    error_smooth_window = error_smooth_window or math.trunc(n * 0.01)
    cfile = (path or "") + "critic_scores.pickle"
    cached_critic = bool(path) and os.path.exists(cfile)

    def critic_branch():
        if cached_critic:
            return np.asarray(_load_pickle(cfile))
        return _compute_critic_score(kde_modes(critic, y_hat.shape[1]), critic_smooth_window)

    def rec_scores_of(kind):
        rec, predictions = reconstruction_errors(y, y_hat, 1, score_window, error_smooth_window, smooth, kind)
        return zscore_clip(rec), predictions

    def rec_branch():
        had_requested = bool(path) and os.path.exists(path + rec_error_type + ".pickle")
        if path:
            for kind in ("point", "area", "dtw"):
                if not os.path.exists(path + kind + ".pickle"):
                    _dump_pickle(rec_scores_of(kind)[0].cpu().numpy(), path + kind + ".pickle")
        if had_requested:
            return np.asarray(_load_pickle(path + rec_error_type + ".pickle")), []
        rec_scores, predictions = rec_scores_of(rec_error_type)
        if path:
            _dump_pickle(rec_scores.cpu().numpy(), path + rec_error_type + ".pickle")
        return rec_scores, predictions

    # the critic smoothing (queued first, on a side stream) runs beside the reconstruction errors (this stream, with the host round
    # trips the reference's NumPy return types ask for)
    if torch.cuda.is_available() and not cached_critic:
        (rec_scores, predictions), critic_scores = concurrently(rec_branch, critic_branch)
    else:
        critic_scores = critic_branch()
        rec_scores, predictions = rec_branch()
    if path and not cached_critic:
        _dump_pickle(critic_scores.cpu().numpy(), cfile)
    final = combine_euclidean(comb, critic_scores, rec_scores)
    # [[t0], [t1], ...] as the reference returns it: 250 000 Python objects at 125 000 windows, 50 ms -- two thirds of the whole detector
    # call; ``with_true=False`` (univariate_anomaly_detection, which drops it like the reference's caller does) returns [] instead
    true = unroll_true(y).cpu().numpy().astype(np.float64).reshape(-1, 1).tolist() if with_true else []
    return final, index, true, predictions


def hyperbolic_scores(recons_signal, true_signal, critic_score, signal_shape, combination="mult", params=None, path=None):
    """The hyperbolic branch of univariate_anomaly_detection (:54-86) up to final_scores (``params`` / ``path``: the
    ``critic_scores.pickle`` cache of compute_critic_scores)."""
    rec = hyperbolic_rec_scores(recons_signal, true_signal, signal_shape)
    critic_scores = []
    if uses_critic(combination):
        critic_scores = compute_critic_scores(rec, critic_score, true_signal, params, path)
    return combine_scores(combination, critic_scores, rec, recons_signal)


def save_result(params, signal, out):
    """:112-126 -- one row [signal, tn, fp, fn, tp] appended to ``./results/<params.filename>`` unless ``params.signal`` already
    has one (the reference's check), the table created with its header when missing."""
    import pandas as pd
    file_place = "./results/{}".format(params.filename)
    os.makedirs(os.path.dirname(file_place), exist_ok=True)
    res = pd.read_csv(file_place) if os.path.isfile(file_place) else pd.DataFrame(columns=["signal", "tn", "fp", "fn", "tp"])
    if params.signal not in list(res["signal"]):
        res.loc[len(res)] = [signal] + list(out)
        res.to_csv(file_place, index=False)
    return file_place


def univariate_anomaly_detection(recons_signal, true_signal, params, combination, critic_score, path=None, read_path=None,
                                 rec_error_type="euclidean", true_index=None, known_anomalies=None, signal=None,
                                 signal_shape=None):
    """:21-127 end to end: window scores on the device, interval extraction and overlap-segment counts on the host.

    The reference's artefacts are written when ``path`` is given -- the score caches (score_anomalies / compute_critic_scores),
    ``path + "anomalies.csv"`` with the predicted intervals, and, with ``params.save_result``, the results table
    (``save_result``).  ``read_path`` is accepted and ignored (the reference reads that CSV only for its timestamp range,
    which the overlap form of the metrics does not use).  The result is returned instead of printed:
        dict(final_scores, intervals (n, 3) [start, end, score], confusion [tn, fp, fn, tp] or [0, 0, 0, 0] when no
        interval was predicted (the reference's except branch), metrics or None)
    """
    if not params.hyperbolic:
        final_scores, true_index, _, _ = score_anomalies(true_signal, recons_signal, critic_score, true_index,
                                                         rec_error_type=rec_error_type, comb=combination, path=path, with_true=False)
    else:
        final_scores = hyperbolic_scores(recons_signal, true_signal, critic_score, params.signal_shape, combination, params, path)
    return detect_intervals(final_scores, params, path, true_index, known_anomalies, signal)


def detect_intervals(final_scores, params, path=None, true_index=None, known_anomalies=None, signal=None, intervals=None):
    """The host tail of univariate_anomaly_detection (:87-127) from the final scores on: intervals, ``anomalies.csv``, the
    overlap-segment counts and metrics, the results table row.  ``intervals``: the signal's (n, 3) rows when they were already
    extracted (find_anomalies_signals on the device); find_anomalies is skipped then."""
    final_scores = np.asarray(final_scores, dtype=np.float64).reshape(-1)
    if true_index is None:
        true_index = np.arange(final_scores.size)
    if intervals is None:
        intervals = find_anomalies(final_scores, true_index, fixed_threshold=True, **UNIVARIATE_INTERVALS)
    out = dict(final_scores=final_scores, intervals=np.asarray(intervals, dtype=np.float64).reshape(-1, 3), confusion=[0, 0, 0, 0],
               metrics=None)
    if path:
        import pandas as pd
        pd.DataFrame(out["intervals"], columns=["start", "end", "score"]).to_csv(path + "anomalies.csv")
    if known_anomalies is not None and out["intervals"].shape[0] > 0:
        pred = [(r[0], r[1]) for r in out["intervals"]]
        out["confusion"] = list(contextual_confusion_matrix(known_anomalies, pred, weighted=False))
        out["metrics"] = compute_metrics(known_anomalies, pred, verbose=False)
    if getattr(params, "save_result", False):
        out["results_file"] = save_result(params, signal, [int(v) for v in out["confusion"]])
    return out


def multivariate_anomaly_detection(recons_signal, true_signal, params, combination, critic_score, path=None, y=None, x_index=None):
    """:129-222 with the ground truth passed in instead of loaded from the reference's data tree (``y``: the 0/1 label
    tensor the reference torch.load()s, or None) and nothing written or plotted.  Reconstruction score: z-scored L2 norm
    (Euclidean) or z-scored row-wise Poincare distance (hyperbolic), on the device; intervals with the multivariate
    settings (window 0.2 T, step 0.1 window, padding 200).  Returns dict(final_scores, intervals, known_anomalies, metrics)."""
    n = len(recons_signal)
    if x_index is None:
        from .dataloader import _yahoo_timestamps       # the reference's stand-in index: one time stamp per second (:133-137)
        x_index = _yahoo_timestamps(n)
    if not params.hyperbolic:
        diff = _f32(np.asarray(true_signal, dtype=np.float32).reshape(n, -1) - np.asarray(recons_signal, dtype=np.float32).reshape(n, -1))
        rec = row_norms(diff)
    else:
        rec = hyperbolic_rec_scores(recons_signal, true_signal, params.signal_shape)
    rec = rec if isinstance(rec, torch.Tensor) else torch.as_tensor(np.asarray(rec, dtype=np.float64))
    rec_scores = zscore_clip(rec.to(torch.float64)).cpu().numpy()
    critic_scores = []
    if uses_critic(combination):
        ts = np.asarray(true_signal)
        critic_scores = final_critic_scores(critic_score, ts.reshape(len(ts), -1))[: rec_scores.shape[0]]
    final_scores = np.asarray(combine_scores(combination, critic_scores, rec_scores, recons_signal), dtype=np.float64).reshape(-1)
    return multivariate_intervals(final_scores, x_index, y)


def multivariate_intervals(final_scores, x_index, y=None, intervals=None):
    """The host tail of multivariate_anomaly_detection (:183-222) from the final scores on: intervals with the multivariate settings
    (window 0.2 T, step 0.1 window, padding 200), CASAS-style ground truth from ``y`` and the overlap-segment metrics.  ``intervals``:
    the signal's (n, 3) rows when they were already extracted (find_anomalies_signals on the device); find_anomalies is skipped then."""
    if intervals is None:
        intervals = find_anomalies(final_scores, x_index, fixed_threshold=True, **MULTIVARIATE_INTERVALS)
    out = dict(final_scores=final_scores, intervals=np.asarray(intervals, dtype=np.float64).reshape(-1, 3), known_anomalies=None, metrics=None)
    if y is not None:
        known = casas_anomalies(y, np.asarray(x_index))
        out["known_anomalies"] = known
        if out["intervals"].shape[0] and len(known):
            out["metrics"] = compute_metrics(known, [(r[0], r[1]) for r in out["intervals"]], verbose=False)
    return out


def zscore_clip_signals(x, seg_off):
    """zscore_clip of every segment [seg_off[s], seg_off[s + 1]) of a device vector in one C call (hypad_zscore_clip_signals: two
    launches per 64 signals): each segment's numbers are zscore_clip's on it alone, bit for bit."""
    seg_off = [int(v) for v in seg_off]
    entries = x.numel() if isinstance(x, torch.Tensor) else np.asarray(x).size
    if entries != seg_off[-1]:
        raise ValueError(f"x has {entries} entries, the offsets say {seg_off[-1]}")
    x = _f64(x).reshape(-1)
    k = len(seg_off) - 1
    out = torch.empty_like(x)
    nbytes = _C.lib.hypad_zscore_clip_signals_workspace_bytes(k)
    ws = _scratch(x.device, nbytes, "zscore_clip_signals")
    _C.check(_C.lib.hypad_zscore_clip_signals(_C.ptr(x), _C.ptr(out), k, _C.int64s(seg_off), ws.data_ptr(), nbytes, _C.stream()),
             "zscore_clip_signals")
    return out


def multivariate_scores_signals(res, true, combination="mult"):
    """multivariate_anomaly_detection (:129-222) up to final_scores for every signal of a score_signals result at once, nothing through
    the host: the reconstruction score of all rows -- the L2 norm of true - recons (row_diff_norms) or, for a hyperbolic result, the
    row-wise Poincare distance between the windows on the ball and the reconstructions --, its z-score per signal
    (zscore_clip_signals), the critic chain per signal (final_critic_scores_signals) where the combination uses it, then the
    combination (hypad_combine_scores_signals).  ``true``: the group's fp32 window matrix on the device, (sum n_s, S) --
    score_signals' ``x``.  Each signal's final_scores are multivariate_anomaly_detection's on it alone, bit for bit (all NaN where
    trunc(n_s * 0.01) is 0 and the critic is used).
    Returns dict(final_scores (sum n_s,), rec_scores (sum n_s,), critic_scores (sum (n_s + S - 1),) or None, row_off); fp64 on the device."""
    if combination not in COMBINATIONS:
        raise ValueError(combination)
    if res.get("hyper_real") is None:
        true, recons = _C.require_cuda(true, "true"), _f32(res["recons"])
        if tuple(true.shape) != tuple(recons.shape):
            raise ValueError(f"true is {tuple(true.shape)}, the reconstructions {tuple(recons.shape)}")
        rec = row_diff_norms(true, recons)
    else:
        rec = _poincare_rowdist_f64(res)
    rec_scores = zscore_clip_signals(rec, res["row_off"])
    return dict(_combine_signals(res, rec_scores, combination), rec_scores=rec_scores)


def final_critic_scores_signals(critic, row_off, window, with_modes=False):
    """final_critic_scores (:365-404) of every signal of a group in one C call (hypad_critic_chain_signals: at most eleven launches
    per 64 signals): ``critic`` the (sum n_s,) window-critic values of all signals in row order on the device, ``row_off`` the host
    offsets, ``window`` the signal shape.  Returns the scores in timestep layout, (sum (n_s + window - 1),) fp64 on the device --
    signal s's are final_critic_scores' on it alone, bit for bit (all NaN where trunc(n_s * 0.01) is 0) -- and with ``with_modes``
    also the KDE modes in the same layout.  Nothing passes through the host."""
    row_off = [int(v) for v in row_off]
    k, w = len(row_off) - 1, int(window)
    entries = critic.numel() if isinstance(critic, torch.Tensor) else np.asarray(critic).size
    if entries != row_off[-1]:
        raise ValueError(f"critic has {entries} entries, the offsets say {row_off[-1]} windows")
    c = _f32(critic).reshape(-1)
    offs = _C.int64s(row_off)
    out = torch.empty(row_off[-1] + k * (w - 1), device=c.device, dtype=torch.float64)
    modes = torch.empty_like(out) if with_modes else None
    nbytes = _C.lib.hypad_critic_chain_signals_workspace_bytes(k, offs, w)
    ws = _scratch(c.device, nbytes, "critic_chain_signals")
    _C.check(_C.lib.hypad_critic_chain_signals(_C.ptr(c), _C.ptr(modes), _C.ptr(out), k, offs, w, ws.data_ptr(), nbytes, _C.stream()),
             "critic_chain_signals")
    return (out, modes) if with_modes else out


def hyperbolic_scores_signals(res, combination="mult"):
    """hyperbolic_scores for every signal of a score_signals result at once (no cache files): the row-wise Poincare distance over all
    rows, per signal the KDE modes of its critic values, its quantile-trimmed |z| + 1 and its own centred rolling mean
    (final_critic_scores_signals: hypad_critic_chain_signals), then the combination (hypad_combine_scores_signals) -- each signal's numbers those of
    hyperbolic_scores on it alone, bit for bit, nothing through the host.
    Returns dict(final_scores (sum n_s,) fp64, critic_scores (sum (n_s + S - 1),) fp64 or None -- signal s's final_critic_scores at
    row_off[s] + s (S - 1) --, row_off) on the device."""
    if combination not in COMBINATIONS:
        raise ValueError(combination)
    if res["hyper_real"] is None:
        raise ValueError("hyperbolic_scores_signals needs a hyperbolic score_signals result")
    return _combine_signals(res, _poincare_rowdist_f64(res), combination)


def _poincare_rowdist_f64(res):
    """Row-wise Poincare distance between the windows on the ball and the reconstructions of a hyperbolic score_signals result, fp64."""
    rec = gmath.poincare_rowdist(_f32(res["hyper_real"]), _f32(res["recons"]))
    return rec if rec.dtype == torch.float64 else rec.to(torch.float64)


def _combine_signals(res, rec, combination):
    """The shared second half of hyperbolic_scores_signals and multivariate_scores_signals: ``rec`` the (sum n_s,) fp64 reconstruction
    score of every row of the score_signals result ``res``; the critic chain per signal where the combination uses it, the row norms of
    the reconstructions where it has "uncertainty", then hypad_combine_scores_signals.  Returns dict(final_scores, critic_scores, row_off)."""
    row_off = [int(v) for v in res["row_off"]]
    recons = _f32(res["recons"])
    w = recons.shape[1]
    critic_scores = final_critic_scores_signals(res["critic"], row_off, w) if uses_critic(combination) else None
    u = row_norms(recons) if "uncertainty" in combination else None
    out = torch.empty(row_off[-1], device=recons.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_combine_scores_signals(_C.COMB[combination], _C.ptr(critic_scores), _C.ptr(rec), _C.ptr(u), _C.ptr(out),
                                                 len(row_off) - 1, _C.int64s(row_off), w, _C.stream()), "combine_signals")
    return {"final_scores": out, "critic_scores": critic_scores, "row_off": row_off}


def timestep_offsets(row_off, S):
    """Timestep layout (include/hypad.h, "Signal groups") of a group with window offsets ``row_off``: signal s owns the
    n_s + S - 1 entries from t_off[s] = row_off[s] + s (S - 1) on.  Host list, len(row_off) entries."""
    return [int(r) + s * (int(S) - 1) for s, r in enumerate(row_off)]


def _upload(a):
    """A host array as a device tensor (one copy)."""
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def unroll_true_signals(x_list, row_off, S):
    """unroll_true (:908-910) of every signal of a group as ONE fp64 device vector in timestep layout.  x_list: per signal a dataset
    (its ``X``) or an (N, S[, 1]) window array.  Gathered on the host from each window matrix in its own dtype -- the first value of
    every window, then the rest of the last one -- and widened to fp64: a pure gather, hence the bits unroll_true gives."""
    S = int(S)
    t_off = timestep_offsets(row_off, S)
    out = np.empty(t_off[-1], dtype=np.float64)
    for s, x in enumerate(x_list):
        X = np.asarray(x.X if hasattr(x, "X") else x)
        X = X.reshape(len(X), -1)
        n = int(row_off[s + 1]) - int(row_off[s])
        if X.shape != (n, S):
            raise ValueError(f"signal {s}: windows {X.shape}, offsets say ({n}, {S})")
        out[t_off[s]: t_off[s] + n] = X[:, 0]
        out[t_off[s] + n: t_off[s + 1]] = X[-1, 1:]
    return _upload(out)


def euclidean_scores_signals(res, true_unrolled, rec_error_type="dtw", comb="mult", kinds=None, score_window=10, with_critic=None):
    """score_anomalies (:407-576, no cache files) for every signal of a Euclidean score_signals result at once, everything in
    timestep layout and nothing through the host: the anti-diagonal medians of all reconstructions (hypad_unroll_median_signals),
    the z-scored reconstruction scores of ``kinds`` (default: the requested one; hypad_rec_scores_signals), beside them the critic
    chain of final_critic_scores (final_critic_scores_signals: hypad_critic_chain_signals; ``with_critic``: default unless comb is
    "rec"), then the combination over the whole vector.  Each signal's numbers are score_anomalies' on it alone, bit for bit.
    ``true_unrolled``: unroll_true_signals of the group.
    Returns dict(final_scores, critic_scores (or None), rec_scores {kind: tensor}, row_off, t_off); tensors fp64 on the device."""
    mode = _euclidean_mode(comb)
    kind = rec_error_type.lower()
    kinds = [kind] if kinds is None else [k.lower() for k in kinds]
    if kind not in kinds:
        kinds.append(kind)
    for k in kinds:
        if k not in _C.REC_KINDS:
            raise ValueError(k)
    if res.get("hyper_real") is not None:
        raise ValueError("euclidean_scores_signals needs a Euclidean score_signals result")
    row_off = [int(v) for v in res["row_off"]]
    k_sig = len(row_off) - 1
    recons = _f32(res["recons"])
    w = recons.shape[1]
    t_off = timestep_offsets(row_off, w)
    total = t_off[-1]
    true = _f64(true_unrolled).reshape(-1)
    if true.numel() != total:
        raise ValueError(f"true_unrolled has {true.numel()} entries, the group {total} timesteps")
    offs = _C.int64s(row_off)
    with_critic = (comb != "rec") if with_critic is None else bool(with_critic) or comb != "rec"
    rec = {k: torch.empty(total, device=recons.device, dtype=torch.float64) for k in kinds}

    def rec_branch():
        median = torch.empty(total, device=recons.device, dtype=torch.float32)
        _C.check(_C.lib.hypad_unroll_median_signals(_C.ptr(recons), _C.ptr(median), k_sig, offs, w, _C.stream()), "unroll_median_signals")
        nbytes = _C.lib.hypad_rec_scores_signals_workspace_bytes(k_sig, offs, w)
        ws = _scratch(recons.device, nbytes, "rec_scores_signals")
        mask = sum(_C.REC_KINDS[k] for k in kinds)
        _C.check(_C.lib.hypad_rec_scores_signals(mask, _C.ptr(true), _C.ptr(median), _C.ptr(rec.get("point")), _C.ptr(rec.get("area")),
                                                 _C.ptr(rec.get("dtw")), k_sig, offs, w, int(score_window), ws.data_ptr(), nbytes, _C.stream()),
                 "rec_scores_signals")
        return rec[kind]

    def critic_branch():
        return final_critic_scores_signals(res["critic"], row_off, w)

    if with_critic:                  # (the critic chain on a side stream beside the reconstruction scores, as score_anomalies runs them)
        r, c = concurrently(rec_branch, critic_branch)
    else:
        r, c = rec_branch(), None
    final = torch.empty(total, device=recons.device, dtype=torch.float64)
    _C.check(_C.lib.hypad_combine_scores(_C.COMB[mode], _C.ptr(c), _C.ptr(r), None, _C.ptr(final), total, _C.stream()), "combine")
    return {"final_scores": final, "critic_scores": c, "rec_scores": rec, "row_off": row_off, "t_off": t_off}


FA_ZERO_WEIGHT, FA_OVERFLOW, FA_INTERNAL = 1, 2, 4         # HYPAD_FA_* (include/hypad.h)


def _per_signal(value, k, name):
    if value is None or np.isscalar(value):
        return [value] * k
    value = list(value)
    if len(value) != k:
        raise ValueError(f"{name}: {len(value)} entries for {k} signals")
    return value


def find_anomalies_signals(scores, seg_off, index_list=None, window_size_portion=None, window_step_size_portion=None, window_size=None,
                           window_step_size=None, min_percent=0.1, anomaly_padding=50, lower_threshold=False, fixed_threshold=True,
                           capacity=64):
    """find_anomalies (:1363-1472, fixed threshold) of every signal of a group in one C call (hypad_find_anomalies_signals: four
    launches per 64 signals, five with ``lower_threshold``) and one copy back.  ``scores``: the fp64 score vector of all signals on the
    device; ``seg_off``: the host offsets of the signals' segments in it -- ``row_off`` for hyperbolic results, ``t_off`` for Euclidean
    ones.  ``window_size`` / ``window_step_size``: one value or one per signal; the portions give each signal's own
    int(np.ceil(n * portion)) as find_anomalies computes them.  ``index_list``: per signal the index its positions are looked up in
    (None: the positions themselves).  A window covered entirely by one padded run whose maximum is not positive reports the
    reference's sentinel row instead, at position window_start - 1; for a signal's first window that is -1, which the lookup reads
    as index[-1] exactly as find_anomalies does.  ``capacity``: table rows per signal of the first attempt; a signal with more intervals makes
    the call run once more with room for the largest count.
    Returns a list of (n_i, 3) float64 arrays [index[start], index[stop], score], one per signal: interval bounds equal
    find_anomalies', scores up to the order of the fp64 sums.  Raises ZeroDivisionError where find_anomalies does (touching
    zero-length sequences, :1302) and ValueError for ``fixed_threshold=False`` (the Nelder-Mead threshold stays on the host)."""
    if not fixed_threshold:
        raise ValueError("find_anomalies_signals computes the fixed threshold only (fixed_threshold=True); the dynamic threshold is "
                         "intervals.find_anomalies on the host")
    seg_off = [int(v) for v in seg_off]
    k = len(seg_off) - 1
    if k < 1:
        raise ValueError("seg_off needs at least two entries")
    if not isinstance(scores, torch.Tensor):
        scores = _upload(np.asarray(scores, dtype=np.float64).reshape(-1))
    scores = _C.require_cuda(scores.reshape(-1), "scores", torch.float64)
    if scores.numel() != seg_off[-1]:
        raise ValueError(f"scores has {scores.numel()} entries, the offsets say {seg_off[-1]}")
    sizes, steps = [], []
    for s, (ws, st) in enumerate(zip(_per_signal(window_size, k, "window_size"), _per_signal(window_step_size, k, "window_step_size"))):
        n = seg_off[s + 1] - seg_off[s]
        ws = ws or n                                         # (the arithmetic of find_anomalies :1420-1428)
        if window_size_portion:
            ws = int(np.ceil(n * window_size_portion))
        st = st or ws
        if window_step_size_portion:
            st = int(np.ceil(ws * window_step_size_portion))
        sizes.append(int(ws))
        steps.append(int(st))
    offs, wsz, wst = _C.int64s(seg_off), _C.int64s(sizes), _C.int64s(steps)
    nbytes = _C.lib.hypad_find_anomalies_signals_workspace_bytes(k, offs, wsz, wst, int(bool(lower_threshold)))
    ws_buf = _scratch(scores.device, nbytes, "find_anomalies_signals")
    capacity = max(int(capacity), 1)
    while True:
        # one buffer, one copy: [tables (k, capacity, 3) fp64 | counts (k,) int32 | status (k,) int32]
        buf = torch.empty(k * capacity * 24 + k * 8, dtype=torch.uint8, device=scores.device)
        base = buf.data_ptr()
        p_counts = base + k * capacity * 24
        _C.check(_C.lib.hypad_find_anomalies_signals(_C.ptr(scores), k, offs, wsz, wst, int(anomaly_padding), float(min_percent),
                                                     int(bool(lower_threshold)), ctypes.c_void_p(base), ctypes.c_void_p(p_counts),
                                                     ctypes.c_void_p(p_counts + k * 4), capacity, ws_buf.data_ptr(), nbytes, _C.stream()),
                 "find_anomalies_signals")
        host = buf.cpu().numpy()
        tables = host[: k * capacity * 24].view(np.float64).reshape(k, capacity, 3)
        counts = host[k * capacity * 24: k * capacity * 24 + k * 4].view(np.int32)
        status = host[k * capacity * 24 + k * 4:].view(np.int32)
        if (status & FA_INTERNAL).any():
            raise _C.HypadError("find_anomalies_signals: a window holds more values above its threshold than the workspace plans for")
        if (status & FA_ZERO_WEIGHT).any():
            raise ZeroDivisionError("Weights sum to zero, can't be normalized")
        if not (status & FA_OVERFLOW).any():
            break
        capacity = int(counts.max())
    out = []
    for s in range(k):
        rows = tables[s, : int(counts[s])].copy()
        if index_list is not None and index_list[s] is not None and rows.shape[0]:
            index = np.asarray(index_list[s])
            rows[:, 0] = index[rows[:, 0].astype(np.int64)]
            rows[:, 1] = index[rows[:, 1].astype(np.int64)]
        out.append(rows)
    return out
