"""Command-line driver (reference: main.py:15-70): YAML config -> datasets -> training -> anomaly detection.

    python -m hypad_amd.main --config configs/univariate.yaml [--data-dir ./data] [--resident | --per-iteration]

Default (and ``--drop-in``, kept as an alias): the reference's own call chain -- ``train.train(train_loader, params, config_path)``
over a shuffling ``DataLoader`` (main.py:33-55) with the reference's host random numbers -- where every epoch runs as one
captured ``hypad_train_epoch`` (``train.train_tadgan``, hypad_amd/epoch_feed.py).  ``--per-iteration`` runs that loop call by
call instead (three iteration functions per minibatch); ``--resident`` draws all randomness and the shuffles on the device
(``train.train_resident``: no host work per epoch at all, a different random stream).  Scoring is the same either way: fused
test-loop forward, device scoring kernels, host interval extraction and overlap-segment metrics.  Prints the metrics and
returns them from ``run``."""
import argparse
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

LATENT_DIM = 20                       # the latent dimension of every model (the reference's train.py:413 sets it, whatever the config says)
Signal = namedtuple("Signal", "params train test read_path name")       # one signal of a run: its params, datasets, CSV path and name


def run(params, config_path=None, data_dir="./data", drop_in=True, log=print, resident=False, per_iteration=False):
    """``drop_in`` (default True) = the reference's call chain over a DataLoader; ``drop_in=False`` or ``resident=True`` = the resident path."""
    resident = resident or not drop_in
    from torch.utils.data import DataLoader

    from . import train as ht
    from .utils import data as od

    log("dataset: {}, signal: {}".format(params.dataset, params.signal))
    train_dataset, test_dataset, read_path = od.dataset_selection(params, data_dir)
    if not resident:
        if per_iteration:
            params.per_iteration = True
        train_loader = DataLoader(train_dataset, batch_size=params.batch_size, drop_last=True, shuffle=True, num_workers=0)
        encoder, decoder, critic_x, _, path = ht.train(train_loader, params, config_path)
    else:                                                              # (utils/dataloader_multivariate.py datasets train on their window matrix)
        resident = train_dataset.device_windows("cpu") if hasattr(train_dataset, "device_windows") else train_dataset
        encoder, decoder, critic_x, _, path, _ = ht.train_resident(resident, params, config_path, log=log)
    multivariate = _multivariate(Signal(params, train_dataset, test_dataset, read_path, params.signal))
    return _detect(params, test_dataset, read_path, encoder, decoder, critic_x, path, data_dir, multivariate, log)


def _detect(params, test_dataset, read_path, encoder, decoder, critic_x, path, data_dir, multivariate, log):
    """main.py:57-70 / anomaly_detection.py:20-155: the test loop and the detector for one trained model."""
    from torch.utils.data import DataLoader

    from . import anomaly_detection
    from .utils import anomaly_detection_utils as adu
    test_loader = DataLoader(test_dataset, batch_size=params.batch_size, drop_last=False, shuffle=False, num_workers=0)
    recons_signal, true_signal, critic_score = anomaly_detection.test_tadgan(
        test_loader, encoder, decoder, critic_x, read_path=read_path, signal=params.signal, path=path, signal_shape=params.signal_shape,
        params=params)
    if multivariate:                                                   # anomaly_detection.py:137-140
        out = adu.multivariate_anomaly_detection(recons_signal, true_signal, params, params.combination, critic_score, path, y=_labels(test_dataset))
    else:
        out = adu.univariate_anomaly_detection(recons_signal, true_signal, params, params.combination, critic_score, path, read_path,
                                               params.rec_error, _true_index(test_dataset, params), _known_anomalies(params, read_path, data_dir),
                                               params.signal, params.signal_shape)
    _log_result(out, log)
    return out


def _labels(test_dataset):
    """The reference torch.load()s the multivariate labels from its data tree (utils/anomaly_detection_utils.py:143-151); the test
    dataset already holds that tensor."""
    return test_dataset.y if len(getattr(test_dataset, "y", [])) else None


def _known_anomalies(params, read_path, data_dir):
    """The labelled intervals of a univariate signal (anomaly_detection.py:32-37)."""
    if params.dataset in ("A1", "A2", "A3", "A4"):
        import pandas as pd
        return pd.read_csv(read_path[:-4] + "_known_anomalies.csv")
    from .utils import data as od
    return od.load_anomalies(params.signal, data_dir=data_dir)


def _log_result(out, log):
    """A detector's result dict as the log lines of a run (the multivariate detector counts no confusion matrix)."""
    log("predicted intervals:\n{}".format(out["intervals"]))
    if "confusion" in out:
        log("tn, fp, fn, tp: {}".format(out["confusion"]))
    if out.get("metrics"):
        log("precision: {precision}, recall: {recall}\nf1_score: {f1}, gmean: {gmean}".format(**out["metrics"]))


def run_signals(params, names, config_path=None, data_dir="./data", log=print, grouped_scoring=True, device_intervals=False):
    """One model per signal for a list of signals (``--signals a,b,c``): datasets -> ``train.train_signals_resident`` (groups of up
    to 32 models per launch sequence; under ``torchrun`` the signals are sharded over the ranks, one process per GPU) -> the test
    loop and the detector on the rank that trained each signal -> the metrics of all signals gathered on every rank.
    ``grouped_scoring`` (default): the signals this rank trained are scored together (_detect_grouped: one grouped forward, the
    hyperbolic critic chain per segment, one copy back; multivariate datasets the same way through multivariate_scores_signals,
    a group being either all multivariate or all univariate), with the same numbers and artefacts as the per-signal ``_detect`` loop
    (``grouped_scoring=False``, ``--per-signal-scoring``).  ``device_intervals`` (``--device-intervals``, grouped scoring only): the
    anomalous intervals of the group come from the device as well (find_anomalies_signals) instead of one host find_anomalies per signal."""
    import copy

    from . import parallel as par
    from . import train as ht
    from .utils import data as od
    sets = []
    for name in names:
        p = copy.copy(params)
        p.signal = name
        sets.append(Signal(p, *od.dataset_selection(p, data_dir), name))
    trained = ht.train_signals_resident([s.train for s in sets], params, names=names, log=log)
    local = {}
    group = [s for s in sets if trained[s.name].get("modules") is not None and _groupable(s, trained[s.name]["path"])]
    if device_intervals and not grouped_scoring:
        raise ValueError("device_intervals needs grouped scoring")
    outs = {}
    if grouped_scoring:                                # (a group is of one kind: window matrices with the multivariate detector, or series)
        for kind in (True, False):
            members = [s for s in group if _multivariate(s) == kind]
            if members:
                outs.update(_detect_grouped(members, trained, data_dir, log, device_intervals=device_intervals))
    for s in sets:
        name = s.name
        mods = trained[name].get("modules")
        if mods is None:
            continue                                   # another rank's signal
        s.params.latent_space_dim = LATENT_DIM
        out = outs.get(name)
        if out is None:
            out = _detect(s.params, s.test, s.read_path, mods[0], mods[1], mods[2], trained[name]["path"], data_dir, _multivariate(s), log)
        # (tn is None in the overlap-segment count)
        local[name] = {"confusion": [None if v is None else int(v) for v in out.get("confusion", [])] or None, "metrics": out.get("metrics"),
                       "n_intervals": int(len(out["intervals"])), "final": trained[name]["final"], "path": trained[name]["path"],
                       "rank": trained[name]["rank"]}
    return par.gather_signal_metrics(local)


def _multivariate(s):
    """A signal that takes the multivariate detector (anomaly_detection.py:137-140): the one place that decides it."""
    return hasattr(s.train, "device_windows") or s.params.signal == "multivariate"


def _groupable(s, path):
    """A signal _detect_grouped scores: a multivariate one with test windows (its detector keeps no score cache), or a univariate
    one in the series view without a score cache that the per-signal detector would read back -- critic_scores.pickle under
    ``params.load``; for a Euclidean model any of the four pickles score_anomalies keeps (``path + "dtw.pickle"`` etc., the names it
    reads).  Those take _detect."""
    import os
    p, test_ds = s.params, s.test
    if _multivariate(s):
        return len(test_ds.X) > 0
    if not hasattr(test_ds, "series_windows"):
        return False
    if getattr(p, "load", False) and path and os.path.exists(os.path.join(path, "critic_scores.pickle")):
        return False
    if not p.hyperbolic and path and any(os.path.exists(path + f + ".pickle") for f in ("critic_scores", "point", "area", "dtw")):
        return False                                   # score_anomalies reads those back whatever params.load says; the group never does
    return test_ds.series_windows("cpu") is not None and len(test_ds.X) > 0


def _detect_grouped(group, trained, data_dir, log, device_intervals=False):
    """_detect for several trained signals of one kind at once, with _detect's numbers, files and output dicts: one score_signals call
    (pack, critic and forward launches for all of them), the final scores of the kind, optionally every signal's intervals from the
    device (``device_intervals``: find_anomalies_signals; the host tails then skip find_anomalies), everything back in one page-locked
    copy and one wait; then per signal on the host the cache files test_tadgan writes, the kind's score pickles and the detector's tail.
    The kinds: multivariate signals (window matrices) -- multivariate_scores_signals on the test sets' ``X``, no pickles,
    multivariate_intervals; univariate hyperbolic models -- hyperbolic_scores_signals, critic_scores.pickle, detect_intervals (anomalies.csv,
    counts, metrics, results row); univariate Euclidean models -- euclidean_scores_signals in timestep layout (the un-roll, the
    reconstruction scores and the critic chain; all three kinds of score when a model directory keeps score_anomalies' pickles),
    detect_intervals.  The (N, S) matrices and the pickles' vectors come back only when some signal has a model directory."""
    from . import anomaly_detection
    from .utils import anomaly_detection_utils as adu
    P0 = group[0].params
    hyp, S = bool(P0.hyperbolic), int(P0.signal_shape)
    multivariate = _multivariate(group[0])
    paths = [trained[s.name]["path"] for s in group]       # (the detector's files are named path + file, as _detect names them)
    keep = any(paths)
    tests = [s.test for s in group]
    res = anomaly_detection.score_signals(tests, [tuple(trained[s.name]["modules"][:3]) for s in group], S, LATENT_DIM, hyp)
    row_off = res["row_off"]
    t_off = adu.timestep_offsets(row_off, S)
    # the kind's scores step: the final scores, the offsets of their segments, the index and the settings of the interval search, and
    # the vectors (timestep layout) a model directory keeps as <name>.pickle
    if multivariate:
        from .utils.dataloader import _yahoo_timestamps
        comb = adu.multivariate_scores_signals(res, res["x"], P0.combination)
        seg_off, settings, pickles = row_off, adu.MULTIVARIATE_INTERVALS, {}
        indices = [_yahoo_timestamps(b - a) for a, b in zip(row_off, row_off[1:])]        # the reference's stand-in index (:133-137)
    else:
        settings = adu.UNIVARIATE_INTERVALS
        indices = [_true_index(s.test, s.params) for s in group]
        if hyp:
            comb = adu.hyperbolic_scores_signals(res, P0.combination)
            seg_off = row_off                                 # (compute_critic_scores' cache holds the signal's whole timestep segment)
            pickles = {} if comb["critic_scores"] is None else {"critic_scores": comb["critic_scores"]}
        else:
            comb = adu.euclidean_scores_signals(res, adu.unroll_true_signals(tests, row_off, S), P0.rec_error, P0.combination,
                                                kinds=("point", "area", "dtw") if keep else None, with_critic=keep or None)
            seg_off = t_off
            pickles = dict(comb["rec_scores"], critic_scores=comb["critic_scores"]) if keep else {}      # (score_anomalies' four caches)
    found = [None] * len(group)
    if device_intervals:
        found = adu.find_anomalies_signals(comb["final_scores"], seg_off, index_list=indices, **settings)
    want = {"final": comb["final_scores"]}
    if keep:                                                  # (some directory wants the test loop's files and the score pickles)
        want.update(pickles, recons=res["recons"], critic=res["critic"])
        if hyp:
            want.update(eucl=res["eucl"], hyper_real=res["hyper_real"])
    host = anomaly_detection._to_host(want)
    outs = {}
    for k, (s, raw) in enumerate(zip(group, paths)):
        a, b = row_off[k], row_off[k + 1]
        if raw:
            anomaly_detection.save_test_outputs(raw, host["recons"][a:b], np.asarray(s.test.X), host["critic"][a:b],
                                                *((host["eucl"][a:b], host["hyper_real"][a:b]) if hyp else ()))
            for f in pickles:
                adu._dump_pickle(host[f][t_off[k]: t_off[k + 1]], raw + f + ".pickle")
        final = host["final"][seg_off[k]: seg_off[k + 1]]
        if multivariate:
            out = adu.multivariate_intervals(final, indices[k], _labels(s.test), intervals=found[k])
        else:
            out = adu.detect_intervals(final, s.params, raw, indices[k], _known_anomalies(s.params, s.read_path, data_dir), s.params.signal,
                                       intervals=found[k])
        _log_result(out, log)
        outs[s.name] = out
    return outs


def _true_index(test_dataset, params):
    """The reference hands the dataset's FULL index to the detector (anomaly_detection.py:127-129: `index[0]`, length N + S): the
    Euclidean branch scores N + S - 1 un-rolled timesteps, so find_anomalies indexes beyond the N window starts.  (The first N
    entries equal X_index, which is all the hyperbolic branch's N window scores need.)"""
    return np.asarray(test_dataset.index)


def main(argv=None):
    import yaml
    ap = argparse.ArgumentParser(description="HypAD on MI355X")
    ap.add_argument("--config", type=str, required=True)
    ap.add_argument("--data-dir", type=str, default="./data")
    ap.add_argument("--drop-in", action="store_true", help="(the default) train.train over a DataLoader with the reference's host-side randomness")
    ap.add_argument("--per-iteration", action="store_true", help="that loop call by call: one critic_x / critic_z / decoder_iteration per minibatch")
    ap.add_argument("--resident", action="store_true", help="device-side randomness and shuffles (train.train_resident)")
    ap.add_argument("--signals", type=str, default=None, help="comma-separated signal names of params.dataset: one model per signal, trained side by "
                                                               "side in groups of up to 32 per GPU (train.train_signals_resident); under torchrun the "
                                                               "signals are sharded over the ranks")
    ap.add_argument("--per-signal-scoring", action="store_true", help="with --signals: score the trained signals one by one (the test loop "
                                                                         "and the detector per signal) instead of as one group")
    ap.add_argument("--device-intervals", action="store_true", help="with --signals and grouped scoring: extract the anomalous intervals of "
                                                                     "the group on the device (find_anomalies_signals) instead of "
                                                                     "one host find_anomalies per signal")
    args = ap.parse_args(argv)
    if args.device_intervals and (not args.signals or args.per_signal_scoring):
        ap.error("--device-intervals needs --signals and grouped scoring (no --per-signal-scoring)")
    params = SimpleNamespace(**yaml.load(open(args.config), Loader=yaml.FullLoader))
    if args.signals:
        import os
        import torch
        import torch.distributed as dist
        own_group = False
        if "RANK" in os.environ and not dist.is_initialized():           # one process per GPU (torchrun): RCCL for the end-of-run gather
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group("nccl", device_id=torch.device("cuda", torch.cuda.current_device()))
            own_group = True
        try:
            res = run_signals(params, [n.strip() for n in args.signals.split(",") if n.strip()], args.config, args.data_dir,
                              grouped_scoring=not args.per_signal_scoring, device_intervals=args.device_intervals)
        finally:
            if own_group:
                dist.destroy_process_group()
        for name, r in sorted(res.items()):
            print(name, r["confusion"], r["metrics"])
        return res
    return run(params, args.config, args.data_dir, resident=args.resident, per_iteration=args.per_iteration)


if __name__ == "__main__":
    main()
