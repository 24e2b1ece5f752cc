#!/usr/bin/env python3
"""Engine.window_series against what it replaces for the same answers, a loop
of window_range(t - w + 1, t, keys) over the outputs (and, at width 1, a loop
of window_read) -> profiles/window_series.json.

Two geometries, one process, the product library (those of tools/range_ab.py):
  large    n_windows 1,024, hll_p 14, 32 services (a 512 MB register ring):
           widths 1, 30 and 256, each over the largest valid first..last
  default  Config() with the workload's 20 services, 8 windows: widths 1 and 4
Each ring is filled once (ends spread over every window, distinct traces, 5 %
ERROR spans over 700 series); 1,000 keys are queried.  Rounds are interleaved
series, loop, series, loop, ...: a round of `series` is `--calls` calls of
window_series (the mean per call is recorded), a round of `loop` is one pass of
window_range over the outputs.  The width-1 window_read loop copies every
window's sketches and leaves the estimates and the point queries to Python:
those are timed apart on one window and are not part of the comparison.

The gate is relative: every series round must be below every loop round, at
every geometry and width (exit status 1 otherwise).  Beside the times the file
records the register bytes the sliding kernel reads under the "registers read
twice" model (once at width 1) and those bytes over the time of a whole call --
a call-level rate that includes the folds, the point queries, the copies of
the answers and the wait.  A time that grows about linearly with the width
would mean the ring is read `width` times.

  python tools/series_ab.py [--rounds 5] [--calls 3] [--out profiles/window_series.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_KEYS = 1000


def measure_width(e, cfg, w0, width, keys, args):
    import numpy as np

    from spanagg import hll_estimate
    from spanagg.sketch import cms_query
    W = cfg.n_windows
    first, last = w0 + width - 1, w0 + W - 1
    n_out = last - first + 1
    r = e.window_series(first, last, width, keys)  # warm both arms, and the two must agree
    same = True
    for t in sorted({first, last, first + n_out // 2}):
        one = e.window_range(t - width + 1, t, keys)
        same = same and bool(np.array_equal(r.hist[t - first], one.hist) and np.array_equal(r.errors[t - first], one.errors)
                             and np.array_equal(r.distinct[t - first], one.distinct))
    rounds = {"series_us_per_call": [], "range_loop_us": []}
    if width == 1:
        rounds["read_loop_us"] = []
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for _ in range(args.calls):
            e.window_series(first, last, width, keys)  # (returns after its own wait on the engine stream)
        rounds["series_us_per_call"].append(round((time.perf_counter() - t0) * 1e6 / args.calls, 1))
        t0 = time.perf_counter()
        for t in range(first, last + 1):
            e.window_range(t - width + 1, t, keys)
        rounds["range_loop_us"].append(round((time.perf_counter() - t0) * 1e6, 1))
        if width == 1:
            t0 = time.perf_counter()
            for t in range(first, last + 1):
                sk = e.window_read(t)
            rounds["read_loop_us"].append(round((time.perf_counter() - t0) * 1e6, 1))
    out = {"width": width, "n_out": n_out, **rounds}
    if width == 1:  # what the read loop leaves to Python, on one window (not in the comparison)
        t0 = time.perf_counter()
        [hll_estimate(row, cfg.hll_p) for row in sk.hll], [cms_query(sk.cms, int(k)) for k in keys]
        out["read_loop_python_us_per_window"] = round((time.perf_counter() - t0) * 1e6, 1)
    loops = [v for k in ("range_loop_us", "read_loop_us") for v in rounds.get(k, [])]
    med = statistics.median(rounds["series_us_per_call"])
    n_in = n_out + width - 1
    reg_bytes = (1 if width == 1 else 2) * ((n_in * cfg.n_services) << cfg.hll_p)
    out.update({"median_series_us_per_call": med, "median_range_loop_us": statistics.median(rounds["range_loop_us"]),
                "range_loop_over_series": [round(min(rounds["range_loop_us"]) / max(rounds["series_us_per_call"]), 1),
                                           round(max(rounds["range_loop_us"]) / min(rounds["series_us_per_call"]), 1)],
                "model_register_bytes": reg_bytes,
                "model_register_gb_per_s_over_call_time": round(reg_bytes / med / 1e3, 1),
                "series_below_every_loop_round": max(rounds["series_us_per_call"]) < min(loops),
                "results_equal": same})
    return out


def measure(name, cfg, spans, widths, args):
    import numpy as np

    from range_ab import make_batch
    from spanagg import Engine
    rng = np.random.default_rng(11)
    pool = rng.integers(1, 2**64, 700, dtype=np.uint64)
    keys = np.concatenate([pool, rng.integers(1, 2**64, N_KEYS - len(pool), dtype=np.uint64)])
    w0 = 176_722_560
    with Engine(cfg) as e:
        e.window_advance(w0)
        for _ in range(spans // 1_000_000):
            e.ingest(make_batch(rng, 1_000_000, cfg, w0, pool))
        e.sync()
        per_width = [measure_width(e, cfg, w0, w, keys, args) for w in widths]
    return {"geometry": name, "n_windows": cfg.n_windows, "n_services": cfg.n_services, "hll_p": cfg.hll_p,
            "spans": spans, "n_keys": N_KEYS, "calls_per_series_round": args.calls, "widths": per_width}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_series.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds")
    from spanagg import Config
    out = [measure("large", Config(n_windows=1024, hll_p=14, n_services=32), 4_000_000, (1, 30, 256), args),
           measure("default", Config(n_services=20), 2_000_000, (1, 4), args)]
    for g in out:
        print("SERIES_AB " + json.dumps(g), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/series_ab.py", "unit": "microseconds (host clock around calls that end in a wait)",
                   "arms": {"series": "Engine.window_series over the largest valid first..last, 1,000 keys",
                            "range_loop": "Engine.window_range(t - w + 1, t, keys) for every output t",
                            "read_loop": "width 1: Engine.window_read for every output (estimates and queries left to Python)"},
                   "histogram_path": "one global atomicAdd per non-zero bin of a workgroup's LDS histogram "
                                     "(per-slice partials with a reduce kernel were not built: no A/B)",
                   "geometries": out}, f, indent=1)
        f.write("\n")
    return 0 if all(w["series_below_every_loop_round"] and w["results_equal"] for g in out for w in g["widths"]) else 1


if __name__ == "__main__":
    sys.exit(main())
