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
from types import SimpleNamespace

import numpy as np


def run(params, config_path=None, data_dir="./data", drop_in=True, log=print, resident=False, per_iteration=False):
    """``drop_in`` (default True) = the reference's call chain over a DataLoader; ``drop_in=False`` or ``resident=True`` = the resident path."""
    resident = resident or not drop_in
    import pandas as pd
    from torch.utils.data import DataLoader

    from . import anomaly_detection
    from . import train as ht
    from .utils import anomaly_detection_utils as adu
    from .utils import data as od

    log("dataset: {}, signal: {}".format(params.dataset, params.signal))
    train_dataset, test_dataset, read_path = od.dataset_selection(params, data_dir)
    multivariate = hasattr(train_dataset, "device_windows")            # utils/dataloader_multivariate.py datasets
    if not resident:
        if per_iteration:
            params.per_iteration = True
        train_loader = DataLoader(train_dataset, batch_size=params.batch_size, drop_last=True, shuffle=True, num_workers=0)
        encoder, decoder, critic_x, _, path = ht.train(train_loader, params, config_path)
    else:
        resident = train_dataset.device_windows("cpu") if multivariate else train_dataset
        encoder, decoder, critic_x, _, path, _ = ht.train_resident(resident, params, config_path, log=log)
    return _detect(params, test_dataset, read_path, encoder, decoder, critic_x, path, data_dir, multivariate, log)


def _detect(params, test_dataset, read_path, encoder, decoder, critic_x, path, data_dir, multivariate, log):
    """main.py:57-70 / anomaly_detection.py:20-155: the test loop and the detector for one trained model."""
    import pandas as pd
    from torch.utils.data import DataLoader

    from . import anomaly_detection
    from .utils import anomaly_detection_utils as adu
    from .utils import data as od
    test_loader = DataLoader(test_dataset, batch_size=params.batch_size, drop_last=False, shuffle=False, num_workers=0)
    recons_signal, true_signal, critic_score = anomaly_detection.test_tadgan(
        test_loader, encoder, decoder, critic_x, read_path=read_path, signal=params.signal, path=path, signal_shape=params.signal_shape,
        params=params)
    if params.signal == "multivariate" or multivariate:                 # anomaly_detection.py:137-140
        # the reference torch.load()s the labels from its data tree (utils/anomaly_detection_utils.py:143-151); the test
        # dataset already holds that tensor
        y = test_dataset.y if len(getattr(test_dataset, "y", [])) else None
        out = adu.multivariate_anomaly_detection(recons_signal, true_signal, params, params.combination, critic_score, path, y=y)
        log("predicted intervals:\n{}".format(out["intervals"]))
        if out.get("metrics"):
            log("precision: {precision}, recall: {recall}\nf1_score: {f1}, gmean: {gmean}".format(**out["metrics"]))
        return out
    if params.dataset in ("A1", "A2", "A3", "A4"):                       # anomaly_detection.py:32-37
        known = pd.read_csv(read_path[:-4] + "_known_anomalies.csv")
    else:
        known = od.load_anomalies(params.signal, data_dir=data_dir)
    out = adu.univariate_anomaly_detection(recons_signal, true_signal, params, params.combination, critic_score, path, read_path,
                                           params.rec_error, _true_index(test_dataset, params), known, params.signal, params.signal_shape)
    log("predicted intervals:\n{}".format(out["intervals"]))
    log("tn, fp, fn, tp: {}".format(out["confusion"]))
    if out["metrics"]:
        log("precision: {precision}, recall: {recall}\nf1_score: {f1}, gmean: {gmean}".format(**out["metrics"]))
    return out


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
        sets.append((p,) + tuple(od.dataset_selection(p, data_dir)))
    trained = ht.train_signals_resident([t[1] for t in sets], params, names=names, log=log)
    local = {}
    group = [(t, name) for t, name in zip(sets, names) if trained[name].get("modules") is not None and _groupable(t, trained[name]["path"])]
    if device_intervals and not grouped_scoring:
        raise ValueError("device_intervals needs grouped scoring")
    outs = {}
    if grouped_scoring:                                # (a group is of one kind: window matrices with the multivariate detector, or series)
        for kind in (True, False):
            members = [g for g in group if _multivariate(g[0]) == kind]
            if members:
                outs.update(_detect_grouped(members, trained, data_dir, log, device_intervals=device_intervals))
    for (p, train_ds, test_ds, read_path), name in zip(sets, names):
        mods = trained[name].get("modules")
        if mods is None:
            continue                                   # another rank's signal
        p.latent_space_dim = 20
        out = outs.get(name)
        if out is None:
            out = _detect(p, test_ds, read_path, mods[0], mods[1], mods[2], trained[name]["path"], data_dir, hasattr(train_ds, "device_windows"), log)
        # (tn is None in the overlap-segment count)
        local[name] = {"confusion": [None if v is None else int(v) for v in out.get("confusion", [])] or None, "metrics": out.get("metrics"),
                       "n_intervals": int(len(out["intervals"])), "final": trained[name]["final"], "path": trained[name]["path"],
                       "rank": trained[name]["rank"]}
    return par.gather_signal_metrics(local)


def _multivariate(t):
    """A signal that takes the multivariate detector (anomaly_detection.py:137-140; _detect's test)."""
    return hasattr(t[1], "device_windows") or t[0].signal == "multivariate"


def _groupable(t, path):
    """A signal _detect_grouped scores: a multivariate one with test windows (its detector keeps no score cache), or a univariate
    one in the series view without a score cache that the per-signal detector would read back -- critic_scores.pickle under
    ``params.load``; for a Euclidean model any of the four pickles score_anomalies keeps (``path + "dtw.pickle"`` etc., the names it
    reads).  Those take _detect."""
    import os
    p, train_ds, test_ds, _ = t
    if _multivariate(t):
        return len(test_ds.X) > 0
    if not hasattr(test_ds, "series_windows"):
        return False
    if getattr(p, "load", False) and path and os.path.exists(os.path.join(path, "critic_scores.pickle")):
        return False
    if not p.hyperbolic and path and any(os.path.exists(path + f + ".pickle") for f in ("critic_scores", "point", "area", "dtw")):
        return False                                   # score_anomalies reads those back whatever params.load says; the group never does
    return test_ds.series_windows("cpu") is not None and len(test_ds.X) > 0


def _detect_grouped(group, trained, data_dir, log, device_intervals=False):
    """_detect for several trained signals at once: one score_signals call (pack, critic and forward launches for all of them), for
    hyperbolic models hyperbolic_scores_signals, everything back in one page-locked copy and one wait; then per signal on the host
    the cache files test_tadgan writes, critic_scores.pickle, and detect_intervals (anomalies.csv, counts, metrics, results row) --
    the same contents as _detect's.  Euclidean models: euclidean_scores_signals (the un-roll, the reconstruction scores -- all three
    kinds when a model directory keeps score_anomalies' pickles -- and the critic chain of all signals, in timestep layout), one
    copy back, then the pickles and detect_intervals per signal; the reconstruction matrix comes back only for recons_signal.pt.
    ``device_intervals``: find_anomalies_signals extracts every signal's intervals from the final scores before the copy back, and
    detect_intervals takes them instead of running find_anomalies.
    Multivariate signals (window matrices): score_signals on the test sets' ``X``, multivariate_scores_signals, the intervals with the
    multivariate settings, one copy back; then per signal the test loop's files and multivariate_intervals -- _detect's output dict."""
    import pickle

    import pandas as pd
    import torch

    from . import anomaly_detection
    from .utils import anomaly_detection_utils as adu
    from .utils import data as od
    P0 = group[0][0][0]
    hyp = bool(P0.hyperbolic)
    S, L = int(P0.signal_shape), 20
    models = [tuple(trained[name]["modules"][:3]) for _, name in group]
    if _multivariate(group[0][0]):
        return _detect_grouped_multivariate(group, trained, models, log, device_intervals)
    res = anomaly_detection.score_signals([t[2] for t, _ in group], models, S, L, hyp)
    row_off = res["row_off"]
    keep = any(trained[name]["path"] for _, name in group)          # (some directory wants the test loop's files and the score pickles)
    want = {"recons": res["recons"], "critic": res["critic"]} if hyp or keep else {}
    if hyp:
        want.update(hyper_real=res["hyper_real"], eucl=res["eucl"])
        comb = adu.hyperbolic_scores_signals(res, P0.combination)
        want["final"] = comb["final_scores"]
        if comb["critic_scores"] is not None:
            want["critic_scores"] = comb["critic_scores"]
    else:
        tests = [t[2] for t, _ in group]
        comb = adu.euclidean_scores_signals(res, adu.unroll_true_signals(tests, row_off, S), P0.rec_error, P0.combination,
                                            kinds=("point", "area", "dtw") if keep else None, with_critic=keep or None)
        t_off = comb["t_off"]
        want["final"] = comb["final_scores"]
        if keep:
            want["critic_scores"] = comb["critic_scores"]
            want.update({kind: v for kind, v in comb["rec_scores"].items()})
    found = [None] * len(group)
    if device_intervals:                                      # (the detector's settings: univariate_anomaly_detection :89-95)
        found = adu.find_anomalies_signals(comb["final_scores"], row_off if hyp else t_off,
                                           index_list=[_true_index(t[2], t[0]) for t, _ in group], window_size_portion=0.33,
                                           window_step_size_portion=0.1)
    host = anomaly_detection._to_host(want)
    outs = {}
    for k, ((p, _, test_ds, read_path), name) in enumerate(group):
        a, b = row_off[k], row_off[k + 1]
        raw = trained[name]["path"]                           # (the detector's files are named raw + file, as _detect names them)
        path = raw + "/" if raw else ""
        gt_signal = np.asarray(test_ds.X)
        if path or hyp:
            recons_signal = host["recons"][a:b]
            critic_score = list(host["critic"][a:b])
        true_signal = host["hyper_real"][a:b] if hyp else gt_signal
        if path:
            torch.save(recons_signal, path + "recons_signal.pt")
            torch.save(gt_signal, path + "gt_signal.pt")
            torch.save(critic_score, path + "critic_score.pt")
            if hyp:
                torch.save(host["eucl"][a:b], path + "eucl_recons.pt")
                torch.save(true_signal, path + "real_hyper.pt")
        if p.dataset in ("A1", "A2", "A3", "A4"):
            known = pd.read_csv(read_path[:-4] + "_known_anomalies.csv")
        else:
            known = od.load_anomalies(p.signal, data_dir=data_dir)
        if hyp:
            if raw and "critic_scores" in host:                # (compute_critic_scores' cache, the signal's whole segment)
                with open(raw + "critic_scores.pickle", "wb") as f:
                    pickle.dump(host["critic_scores"][a + k * (S - 1): b + (k + 1) * (S - 1)], f, protocol=pickle.HIGHEST_PROTOCOL)
            out = adu.detect_intervals(host["final"][a:b], p, raw, _true_index(test_ds, p), known, p.signal, intervals=found[k])
        else:
            ta, tb = t_off[k], t_off[k + 1]
            if raw:                                            # (score_anomalies' caches: the arrays and the protocol it writes)
                for f in ("critic_scores", "point", "area", "dtw"):
                    adu._dump_pickle(host[f][ta:tb].copy(), raw + f + ".pickle")
            out = adu.detect_intervals(host["final"][ta:tb], p, raw, _true_index(test_ds, p), known, p.signal, intervals=found[k])
        log("predicted intervals:\n{}".format(out["intervals"]))
        log("tn, fp, fn, tp: {}".format(out["confusion"]))
        if out["metrics"]:
            log("precision: {precision}, recall: {recall}\nf1_score: {f1}, gmean: {gmean}".format(**out["metrics"]))
        outs[name] = out
    return outs


def _detect_grouped_multivariate(group, trained, models, log, device_intervals):
    """The multivariate branch of _detect_grouped."""
    import torch

    from . import anomaly_detection
    from .utils import anomaly_detection_utils as adu
    from .utils.dataloader import _yahoo_timestamps
    P0 = group[0][0][0]
    hyp = bool(P0.hyperbolic)
    S = int(P0.signal_shape)
    res = anomaly_detection.score_signals([t[2] for t, _ in group], models, S, 20, hyp)       # (no series view: the X matrices)
    row_off = res["row_off"]
    comb = adu.multivariate_scores_signals(res, res["x"], P0.combination)
    indices = [_yahoo_timestamps(row_off[k + 1] - row_off[k]) for k in range(len(group))]      # the reference's stand-in index (:133-137)
    found = [None] * len(group)
    if device_intervals:                                      # (the detector's settings: multivariate_anomaly_detection :183-187)
        found = adu.find_anomalies_signals(comb["final_scores"], row_off, index_list=indices, window_size_portion=0.2,
                                           window_step_size_portion=0.1, anomaly_padding=200)
    want = {"final": comb["final_scores"]}
    if any(trained[name]["path"] for _, name in group):       # (some directory wants the test loop's files)
        want.update(recons=res["recons"], critic=res["critic"])
        if hyp:
            want.update(hyper_real=res["hyper_real"], eucl=res["eucl"])
    host = anomaly_detection._to_host(want)
    outs = {}
    for k, ((p, _, test_ds, _), name) in enumerate(group):
        a, b = row_off[k], row_off[k + 1]
        raw = trained[name]["path"]
        if raw:                                               # test_tadgan's cache files
            path = raw + "/"
            torch.save(host["recons"][a:b], path + "recons_signal.pt")
            torch.save(np.asarray(test_ds.X), path + "gt_signal.pt")
            torch.save(list(host["critic"][a:b]), path + "critic_score.pt")
            if hyp:
                torch.save(host["eucl"][a:b], path + "eucl_recons.pt")
                torch.save(host["hyper_real"][a:b], path + "real_hyper.pt")
        y = test_ds.y if len(getattr(test_ds, "y", [])) else None
        out = adu.multivariate_intervals(host["final"][a:b], indices[k], y, intervals=found[k])
        log("predicted intervals:\n{}".format(out["intervals"]))
        if out.get("metrics"):
            log("precision: {precision}, recall: {recall}\nf1_score: {f1}, gmean: {gmean}".format(**out["metrics"]))
        outs[name] = out
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
