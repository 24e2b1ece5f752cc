#!/usr/bin/env python3
"""Engine.window_top against what a caller does without it: window_range over
every series the host knows, then RangeResult.top_errors on the host
-> profiles/window_top.json.

Three engines, one process, the product library:
  c4_default  the C4 shape (synth.generate_highcard: 1,000,000 series, binned
              table of key_capacity 1,200,000, 16 windows), count-min 4 x 2,048
  c4_wide     the same with a count-min of 4 x 65,536
  c2_default  synth.generate_c2 on Config() with its services, 16 windows
Each engine ingests its spans once and is never flushed (a flush may reclaim
the key table: the candidates).  The baseline's keys are the distinct series
of the spans ingested -- the vocabulary a detector holds -- so both legs rank
the same series, and their top 10 must be equal.

Rounds are interleaved top, range, top, range, ...: a round of `top` is
`--calls` calls of window_top(first, last, 10) (the mean per call is
recorded), a round of `range` is `--range-calls` calls of window_range(first,
last, keys) each followed by top_errors(10).  Both end in the engine's own
wait, so the host clock around them measures whole calls.  The file records
every round, the median and the range per leg, and whether window_top was
faster in every round; nothing is gated on the times.

  python tools/top_ab.py [--rounds 5] [--calls 20] [--range-calls 1] [--out profiles/window_top.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))

K = 10


def legs(rounds):
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in rounds.items()}


def measure(name, cfg, batch, first, args):
    import numpy as np

    from spanagg import Engine
    keys = np.unique(batch.key_hash)
    keys = keys[keys != 0]
    last = first + cfg.n_windows - 1
    with Engine(cfg) as e:
        e.window_advance(first)
        for a in range(0, len(batch), 1_000_000):
            e.ingest(batch.slice(a, min(len(batch), a + 1_000_000)))
        e.sync()
        t = e.window_top(first, last, K)  # warm both legs, and the two must agree
        r = e.window_range(first, last, keys)
        same = t.items() == r.top_errors(K) and t.n_resident == len(keys)
        geometry = e.debug_geometry()
        rounds = {"top_us_per_call": [], "range_then_host_top_us_per_call": [], "of_which_window_range_us": []}
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                e.window_top(first, last, K)
            rounds["top_us_per_call"].append(round((time.perf_counter() - t0) * 1e6 / args.calls, 1))
            t0, in_range = time.perf_counter(), 0.0
            for _ in range(args.range_calls):
                t1 = time.perf_counter()
                r = e.window_range(first, last, keys)
                in_range += time.perf_counter() - t1
                r.top_errors(K)
            rounds["range_then_host_top_us_per_call"].append(round((time.perf_counter() - t0) * 1e6 / args.range_calls, 1))
            rounds["of_which_window_range_us"].append(round(in_range * 1e6 / args.range_calls, 1))
    return {"engine": name, "path": geometry["path"], "table_slots": 1 << geometry["log2cap"], "spans": len(batch),
            "series": len(keys), "cms_d": cfg.cms_d, "cms_w": cfg.cms_w, "n_windows": cfg.n_windows, "k": K,
            "n_resident": t.n_resident, "n_matched": t.n_matched, "error_spans": t.error_spans,
            "largest_estimate": int(t.errors[0]) if len(t.errors) else 0,
            "calls_per_top_round": args.calls, "calls_per_range_round": args.range_calls, **rounds, "legs": legs(rounds),
            "key_bytes_up_and_estimate_bytes_down_per_range_call": 16 * len(keys),
            "top_faster_every_round": all(a < b for a, b in zip(rounds["top_us_per_call"],
                                                                 rounds["range_then_host_top_us_per_call"])),
            "top_faster_than_window_range_alone_every_round": all(
                a < b for a, b in zip(rounds["top_us_per_call"], rounds["of_which_window_range_us"])),
            "results_equal": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--range-calls", type=int, default=1)
    ap.add_argument("--c4-spans", type=int, default=4_000_000)
    ap.add_argument("--c2-spans", type=int, default=2_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_top.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds")
    from spanagg import Config
    from spanagg.synth import generate_c2, generate_highcard
    hc, _, hc_first = generate_highcard(args.c4_spans, seed=7)
    c2 = generate_c2(args.c2_spans, seed=42)
    c4 = dict(n_services=1, n_windows=16, key_capacity=1_200_000)
    out = [measure("c4_default", Config(**c4), hc, hc_first, args),
           measure("c4_wide", Config(cms_w=65536, **c4), hc, hc_first, args),
           measure("c2_default", Config(n_services=c2.n_services, n_windows=16), c2.batch, c2.first_window, args)]
    for g in out:
        print("TOP_AB " + json.dumps(g), flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/top_ab.py", "unit": "microseconds (host clock around calls that end in a wait)",
                   "legs": {"top": "Engine.window_top(first, last, 10) over the full ring",
                            "range_then_host_top": "Engine.window_range(first, last, every series ingested) "
                                                   "+ RangeResult.top_errors(10)"},
                   "engines": out}, f, indent=1)
        f.write("\n")
    return 0 if all(g["results_equal"] for g in out) else 1


if __name__ == "__main__":
    sys.exit(main())
