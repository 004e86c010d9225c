"""Interval extraction of a scored signal group: the host find_anomalies loop (utils/intervals.py, one call per signal) against
find_anomalies_signals (hypad_find_anomalies_signals: four launches per 64 signals and one copy back).

Workloads, all with the univariate detector's settings (window 0.33 T, step 0.1 window, padding 50, fixed threshold): 32 signals of
1 400 - 2 000 timesteps, one signal of 125 000, one of 10^6; seeded noise plus spikes.  Both sides start from scores that are where
the pipeline leaves them for that side -- on the host for the host loop, on the device for the device call -- and end with the
per-signal (n, 3) arrays on the host, so the device time includes its copy back and the table -> array conversion.  Wall clock
around work that ends synchronised; one warm-up round, then ``--runs`` rounds alternating the two sides; the median and the spread
(min, max) of each side are kept.  Writes profiles/find_anomalies_signals.json, stamped with build.source_digest().

    python scripts/time_find_anomalies.py [--runs 7] [--out profiles/find_anomalies_signals.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def series(n, spikes, width, seed):
    r = np.random.default_rng(seed)
    e = 1.0 + 0.1 * np.abs(r.standard_normal(n))
    for _ in range(spikes):
        c = int(r.integers(0, n))
        e[c: c + int(r.integers(1, width + 1))] += r.uniform(0.8, 3.0)
    return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", type=str, default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                            "find_anomalies_signals.json"))
    args = ap.parse_args()
    if args.runs < 5:
        ap.error("--runs: at least five")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures on the device and has no fallback")
    from hypad_amd import build
    from hypad_amd.utils import anomaly_detection_utils as adu
    from hypad_amd.utils import intervals as iv
    KW = dict(window_size_portion=0.33, window_step_size_portion=0.1)
    rng = np.random.default_rng(0)
    workloads = {
        "32 signals x 1400-2000": [series(int(n), 3, 30, 100 + k) for k, n in enumerate(rng.integers(1400, 2001, size=32))],
        "1 signal x 125000": [series(125_000, 20, 200, 200)],
        "1 signal x 1000000": [series(1_000_000, 40, 300, 300)],
    }
    result = {"source_digest": build.source_digest(), "device": torch.cuda.get_device_name(0), "runs": args.runs, "settings": dict(KW, anomaly_padding=50),
              "timing": "wall clock, device side synchronised by its copy back; one warm-up round, sides alternated", "workloads": {}}
    for name, segs in workloads.items():
        off = [0] + [int(v) for v in np.cumsum([len(s) for s in segs])]
        dev = torch.from_numpy(np.concatenate(segs)).cuda()
        torch.cuda.synchronize()

        def run_host():
            return [np.asarray(iv.find_anomalies(s, np.arange(s.size), fixed_threshold=True, **KW), dtype=np.float64).reshape(-1, 3) for s in segs]

        def run_device():
            return adu.find_anomalies_signals(dev, off, **KW)
        want, got = run_host(), run_device()                      # warm-up, and the results must agree before a time means anything
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a[:, :2], b[:, :2]) and np.allclose(a[:, 2], b[:, 2], rtol=1e-9, atol=0), name
        th, td = [], []
        for _ in range(args.runs):
            t0 = time.perf_counter(); run_host(); t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter(); run_device(); t3 = time.perf_counter()
            th.append((t1 - t0) * 1e3)
            td.append((t3 - t2) * 1e3)
        row = {"signals": len(segs), "timesteps": off[-1], "intervals": int(sum(len(w) for w in want)),
               "host_ms": {"median": float(np.median(th)), "min": min(th), "max": max(th)},
               "device_ms": {"median": float(np.median(td)), "min": min(td), "max": max(td)}}
        row["ratio_median"] = row["host_ms"]["median"] / row["device_ms"]["median"]
        row["ratio_worst"] = row["host_ms"]["min"] / row["device_ms"]["max"]          # slowest device run against the fastest host run
        result["workloads"][name] = row
        print(name, json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
