"""Scoring a group of trained hyperbolic signals: the grouped path (score_signals + hyperbolic_scores_signals, one copy back) against the
per-signal loop (score_windows + hyperbolic_scores per signal, as main._detect runs it), from trained models to final scores on the host.
    python scripts/time_score_signals.py [--cases 1000,5000,20000,ragged] [--reps 5] [--only grouped|per_signal]
``--euclidean [--rec-error dtw] [--all-kinds]``: Euclidean (TadGAN) models instead -- per_signal = the grouped forward, one copy back and
score_anomalies per signal (what _detect_grouped ran before the grouped Euclidean detector), grouped = score_signals +
euclidean_scores_signals and one copy back; --all-kinds scores point, area and dtw as a run with model directories does.
Prints one JSON line per case: median wall ms of each path over --reps (after one warm-up) with the spread of the repetitions, and
whether the final scores are equal bit for bit.  ``--chain``: the critic-score chain alone on the same cases -- per_segment =
hypad_kde_mode_signals + hypad_critic_score_signals (one set of launches per signal), segmented = hypad_critic_chain_signals; seeded
critic values on the device, device tensors in and out, one synchronise at the end of each repetition.  Launch counts: run one case under `rocprofv3 --kernel-trace --stats -- python scripts/time_score_signals.py --cases ragged
--reps 1 --only grouped` (and --only per_signal).
``--multivariate [--signals 8,32]``: multivariate signals (window matrices, S = 150, 600-2 000 windows each), hyperbolic and Euclidean
models -- per_signal = score_windows, one copy back and multivariate_anomaly_detection per signal (main._detect's loop), grouped =
score_signals + multivariate_scores_signals, one copy back and the host interval search per signal (main._detect_grouped),
grouped_device = the same with find_anomalies_signals on the device.  ``--reps 0`` runs each selected path once and times nothing
(for a kernel trace that holds one pass)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

S, L = 100, 20


def _case(name, rng):
    if name == "ragged":
        return [int(v) for v in rng.integers(1_500, 9_001, size=32)]
    return [int(name)] * 32


def chain_alone(args):
    """The critic-score chain of a group without the forward, the combination and the copy back."""
    from hypad_amd import _C
    rng = np.random.default_rng(0)
    for case in args.cases.split(","):
        counts = _case(case, rng)
        row_off = [int(v) for v in np.cumsum([0] + counts)]
        k = len(counts)
        offs = _C.int64s(row_off)
        critic = torch.randn(row_off[-1], device="cuda", generator=torch.Generator(device="cuda").manual_seed(0))
        total = row_off[-1] + k * (S - 1)
        modes, out = (torch.empty(total, device="cuda", dtype=torch.float64) for _ in range(2))
        nb_old = _C.lib.hypad_critic_score_signals_workspace_bytes(k, offs, S)
        nb_new = _C.lib.hypad_critic_chain_signals_workspace_bytes(k, offs, S)
        ws = torch.empty(max(nb_old, nb_new), dtype=torch.uint8, device="cuda")

        def per_segment():
            _C.check(_C.lib.hypad_kde_mode_signals(_C.ptr(critic), _C.ptr(modes), k, offs, S, _C.stream()), "kde_mode_signals")
            _C.check(_C.lib.hypad_critic_score_signals(_C.ptr(modes), _C.ptr(out), k, offs, S, ws.data_ptr(), nb_old, _C.stream()),
                     "critic_score_signals")

        def segmented():
            _C.check(_C.lib.hypad_critic_chain_signals(_C.ptr(critic), _C.ptr(modes), _C.ptr(out), k, offs, S, ws.data_ptr(), nb_new, _C.stream()),
                     "critic_chain_signals")

        row = {"case": case, "chain_only": True, "signals": k, "windows": int(sum(counts))}
        results = {}
        for name, fn in (("per_segment", per_segment), ("segmented", segmented)):
            if args.only and name != args.only:
                continue
            fn()
            torch.cuda.synchronize()
            results[name] = (modes.clone(), out.clone())
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            row[name + "_ms"] = round(float(np.median(ts)), 3)
            row[name + "_min_max_ms"] = [round(float(min(ts)), 3), round(float(max(ts)), 3)]
        if len(results) == 2:
            row["bit_equal"] = all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(results["per_segment"], results["segmented"]))
            row["speedup"] = round(row["per_segment_ms"] / row["segmented_ms"], 2)
        print(json.dumps(row), flush=True)


def multivariate(args):
    """Grouped multivariate scoring against the per-signal loop, from trained models to final scores and intervals on the host."""
    from types import SimpleNamespace

    from hypad_amd import anomaly_detection as ad
    from hypad_amd.models import tadgan
    from hypad_amd.utils import anomaly_detection_utils as adu
    from hypad_amd.utils.dataloader import _yahoo_timestamps
    W = 150
    rng = np.random.default_rng(0)
    for n_sig in [int(v) for v in args.signals.split(",")]:
        counts = [int(v) for v in rng.integers(600, 2_001, size=n_sig)]
        xs = []
        for k, n in enumerate(counts):
            t = np.arange(n)[:, None] * 0.07 + np.arange(W)[None, :] * (0.11 + 0.002 * k)
            x = np.clip(np.sin(t) + 0.1 * rng.standard_normal((n, W)), -1, 1)
            x[n // 2: n // 2 + 20] *= -0.5                      # a stretch that reconstructs badly
            xs.append(x)                                        # fp64 windows, as MultivariateDataset.X holds them
        index = [_yahoo_timestamps(n) for n in counts]
        for hyp in (True, False):
            models = []
            for k in range(n_sig):
                torch.manual_seed(k)
                models.append(tuple(m.cuda().eval() for m in (tadgan.Encoder(W, L), tadgan.Decoder(W, L, hyp), tadgan.CriticX(W, L))))
            P = SimpleNamespace(hyperbolic=hyp, signal_shape=W)

            def per_signal():
                out = []
                for k in range(n_sig):
                    r = ad.score_windows(torch.from_numpy(xs[k]), *models[k], W, L, hyp)
                    want = {"recons": r["recons"], "critic": r["critic"]}
                    if hyp:
                        want["hyper_real"] = r["hyper_real"]
                    host = ad._to_host(want)
                    out.append(adu.multivariate_anomaly_detection(host["recons"], host["hyper_real"] if hyp else xs[k], P, "mult",
                                                                  list(host["critic"])))
                return out

            def grouped(device_intervals=False):
                r = ad.score_signals(xs, models, W, L, hyp)
                f = adu.multivariate_scores_signals(r, r["x"], "mult")
                ro = r["row_off"]
                found = [None] * n_sig
                if device_intervals:
                    found = adu.find_anomalies_signals(f["final_scores"], ro, index_list=index, window_size_portion=0.2,
                                                       window_step_size_portion=0.1, anomaly_padding=200)
                final = ad._to_host({"final": f["final_scores"]})["final"]
                return [adu.multivariate_intervals(final[ro[k]: ro[k + 1]].copy(), index[k], intervals=found[k]) for k in range(n_sig)]

            row = {"multivariate": True, "hyperbolic": hyp, "signals": n_sig, "windows": int(sum(counts)), "S": W}
            results = {}
            for name, fn in (("per_signal", per_signal), ("grouped", grouped), ("grouped_device", lambda: grouped(True))):
                if args.only and name != args.only:
                    continue
                results[name] = fn()
                ts = []
                for _ in range(args.reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t0) * 1e3)
                if ts:
                    row[name + "_ms"] = round(float(np.median(ts)), 3)
                    row[name + "_min_max_ms"] = [round(float(min(ts)), 3), round(float(max(ts)), 3)]
            if "per_signal" in results:
                ref = results["per_signal"]
                for name in ("grouped", "grouped_device"):
                    if name in results:
                        got = results[name]
                        row[name + "_bit_equal"] = all(a["final_scores"].tobytes() == b["final_scores"].tobytes() for a, b in zip(got, ref))
                        row[name + "_same_bounds"] = all(np.array_equal(a["intervals"][:, :2], b["intervals"][:, :2]) for a, b in zip(got, ref))
                        if name + "_ms" in row and "per_signal_ms" in row:
                            row[name + "_speedup"] = round(row["per_signal_ms"] / row[name + "_ms"], 2)
            print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="1000,5000,20000,ragged")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--euclidean", action="store_true")
    ap.add_argument("--rec-error", default="dtw")
    ap.add_argument("--all-kinds", action="store_true")
    ap.add_argument("--chain", action="store_true")
    ap.add_argument("--multivariate", action="store_true")
    ap.add_argument("--signals", default="8,32", help="--multivariate: group sizes")
    args = ap.parse_args()
    if args.chain:
        return chain_alone(args)
    if args.multivariate:
        return multivariate(args)
    from hypad_amd import anomaly_detection as ad
    from hypad_amd.models import tadgan
    from hypad_amd.utils import anomaly_detection_utils as adu
    rng = np.random.default_rng(0)
    for case in args.cases.split(","):
        counts = _case(case, rng)
        models = []
        for k in range(len(counts)):
            torch.manual_seed(k)
            models.append(tuple(m.cuda().eval() for m in (tadgan.Encoder(S, L), tadgan.Decoder(S, L, not args.euclidean), tadgan.CriticX(S, L))))
        series = []
        for k, n in enumerate(counts):
            t = np.arange(n + S - 1)
            series.append(torch.from_numpy(np.clip(np.sin(t * 2 * np.pi / (40 + k)) + 0.1 * rng.standard_normal(n + S - 1), -1, 1)
                                           .astype(np.float32)).cuda())

        class _View:
            def __init__(self, s, n):
                self.s, self.n = s, n

            def series_windows(self, device="cuda"):
                return self.s, self.n, 1

        def per_signal():
            out = []
            for k, n in enumerate(counts):
                r = ad.score_windows(torch.empty(n, S), *models[k], S, L, True, series=series[k])
                host = ad._to_host({"recons": r["recons"], "critic": r["critic"], "hyper_real": r["hyper_real"]})
                out.append(np.asarray(adu.hyperbolic_scores(host["recons"], host["hyper_real"], list(host["critic"]), S, "mult")))
            return np.concatenate(out)

        def grouped():
            r = ad.score_signals([_View(s, n) for s, n in zip(series, counts)], models, S, L, True)
            f = adu.hyperbolic_scores_signals(r, "mult")
            return ad._to_host({"final": f["final_scores"]})["final"].copy()

        if args.euclidean:
            # the datasets' window matrices (fp64, host) -- what score_anomalies un-rolls per signal and unroll_true_signals gathers
            xs = [s.double().cpu().numpy()[np.arange(n)[:, None] + np.arange(S)[None, :]][:, :, None] for s, n in zip(series, counts)]
            kinds = ("point", "area", "dtw")

            def per_signal():
                r = ad.score_signals([_View(s, n) for s, n in zip(series, counts)], models, S, L, False)
                host = ad._to_host({"recons": r["recons"], "critic": r["critic"]})
                ro, out = r["row_off"], []
                for k in range(len(counts)):
                    y_hat, critic = host["recons"][ro[k]: ro[k + 1]], list(host["critic"][ro[k]: ro[k + 1]])
                    if args.all_kinds:                  # (score_anomalies with a model directory: every kind for its pickle, then the requested one)
                        for kind in kinds:
                            adu.zscore_clip(adu.reconstruction_errors(xs[k], y_hat, 1, 10, int(counts[k] * 0.01), True, kind)[0]).cpu().numpy()
                    out.append(adu.score_anomalies(xs[k], y_hat, critic, None, rec_error_type=args.rec_error, comb="mult", with_true=False)[0])
                return np.concatenate(out)

            def grouped():
                r = ad.score_signals([_View(s, n) for s, n in zip(series, counts)], models, S, L, False)
                f = adu.euclidean_scores_signals(r, adu.unroll_true_signals(xs, r["row_off"], S), args.rec_error, "mult",
                                                 kinds=kinds if args.all_kinds else None)
                want = {"final": f["final_scores"]}
                if args.all_kinds:
                    want.update(f["rec_scores"], critic_scores=f["critic_scores"])
                return ad._to_host(want)["final"].copy()

        row = {"case": case, "signals": len(counts), "windows": int(sum(counts))}
        if args.euclidean:
            row.update(euclidean=True, rec_error=args.rec_error, all_kinds=args.all_kinds)
        finals = {}
        for name, fn in (("per_signal", per_signal), ("grouped", grouped)):
            if args.only and name != args.only:
                continue
            finals[name] = fn()
            ts = []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
            row[name + "_ms"] = round(float(np.median(ts)), 3)
            row[name + "_min_max_ms"] = [round(float(min(ts)), 3), round(float(max(ts)), 3)]
        if len(finals) == 2:
            row["bit_equal"] = finals["grouped"].tobytes() == finals["per_signal"].tobytes()
            row["speedup"] = round(row["per_signal_ms"] / row["grouped_ms"], 2)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
