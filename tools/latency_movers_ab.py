#!/usr/bin/env python3
"""What sa_window_latency_movers takes against what the engine offered for the
same answer before it -> profiles/window_latency_movers.json.

One process, one engine per shape.  Two arms give the same rows:

  movers       one window_latency_movers call (k = 10, quantiles 0.99, 0.5, 0.95)
  two_queries  two window_latency range queries over every service, both
               answers on the host, shifts and ranking in numpy

A round is `--reps` calls of one arm, its figure the mean wall time per call;
rounds are interleaved movers, two_queries, movers, ...; the record is each
arm's median round with the rounds' range.  Shapes:

  default  the default engine's ring with the option on: 64 services x 8
           windows, the ranges its two halves
  long     1,024 windows x 32 services (a 64 MiB ring), ranges of 512 windows
  wide     65,536 services x 4 windows (the 512 MiB ring), ranges of 2 windows

`--profile` runs the movers arm alone, `--reps` calls a shape and nothing else
on the device, for a kernel trace taken around it (rocprofv3 --kernel-trace
--stats, no counters); `--kernel-trace <csv>` then adds the sums kernel's own
time per shape -- the median of its dispatches, in the shapes' order -- against
the ring bytes it reads to the record.  No pass or fail time is fixed.

  python tools/latency_movers_ab.py [--rounds 5] [--reps 20] [--kernel-trace run_kernel_trace.csv]
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))
sys.path.insert(0, ROOT)

Q = (0.99, 0.5, 0.95)
K = 10
SHAPES = (("default", 64, 8, 4, 400_000), ("long", 32, 1024, 512, 4_000_000), ("wide", 65_536, 4, 2, 4_000_000))
SUMS_KERNEL = "lat_range_sums_kernel"


def load(S, W, n):
    """An engine of S services x W windows with n spans: ends uniform over the
    ring, durations log-uniform times a factor drawn per (service, window)."""
    import numpy as np

    from spanagg import Config, Engine, SpanBatch, pack_meta
    from spanagg._lib import OPT_WINDOW_LATENCY

    # (the default shape is Config()'s own geometry; the others keep the sketches small)
    cfg = Config(n_services=S, n_windows=W, hll_p=14 if (S, W) == (64, 8) else 4, key_capacity=1000, device=0,
                 options=OPT_WINDOW_LATENCY)
    rng = np.random.default_rng(S + W)
    w0 = 1_000_000
    svc, win = rng.integers(0, S, n), rng.integers(0, W, n)
    end = (np.uint64(w0) + win.astype(np.uint64)) * np.uint64(cfg.window_ns) + rng.integers(0, cfg.window_ns, n, dtype=np.uint64)
    factor = np.exp2(rng.uniform(-2, 2, (S, W)))
    dur = (np.exp(rng.uniform(np.log(1e3), np.log(1e9), n)) * factor[svc, win]).astype(np.uint64)
    key = rng.integers(1, 1000, n).astype(np.uint64)
    tr = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    e = Engine(cfg)
    e.window_advance(w0)
    e.ingest(SpanBatch(key, end - dur, end, tr, tr, pack_meta(svc, np.zeros(n), np.zeros(n))))
    e.sync()
    return e, w0


def two_queries(e, base, cur):
    """The rows of window_latency_movers(base, cur, K, Q) from two range queries."""
    import numpy as np

    b, c = e.window_latency(*base, quantiles=Q), e.window_latency(*cur, quantiles=Q)
    cb, cc = b.count[0], c.count[0]
    shift = c.q_bin[0, :, 0].astype(np.int64) - b.q_bin[0, :, 0].astype(np.int64)
    match = np.flatnonzero((cb >= 1) & (cc >= 1) & (shift >= 1))
    order = match[np.lexsort((match, -np.minimum(cc[match], np.uint64((1 << 48) - 1)).astype(np.int64), -shift[match]))][:K]
    return order, shift[order], cb[order], cc[order], b.q_bin[0, order], c.q_bin[0, order], len(match)


def kernel_times(path, reps):
    """us of the sums kernel's dispatches in a rocprofv3 kernel-trace CSV, `reps` a shape in the shapes' order."""
    with open(path, newline="") as f:
        rows = [r for r in csv.DictReader(f) if SUMS_KERNEL in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    if len(us) != reps * len(SHAPES):
        raise SystemExit(f"{path}: {len(us)} dispatches of {SUMS_KERNEL}, expected {reps} a shape")
    return {name: us[i * reps:(i + 1) * reps] for i, (name, *_) in enumerate(SHAPES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--profile", action="store_true", help="the movers arm alone, for a kernel trace around the run")
    ap.add_argument("--kernel-trace", default=None, help="the kernel-trace CSV of a --profile run with the same --reps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_latency_movers.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds per arm")
    import numpy as np

    traced = kernel_times(args.kernel_trace, args.reps) if args.kernel_trace else None
    parts = []
    for name, S, W, length, n in SHAPES:
        e, w0 = load(S, W, n)
        with e:
            base, cur = (w0, w0 + length - 1), (w0 + W - length, w0 + W - 1)
            arms = {"movers": lambda: e.window_latency_movers(base, cur, K, Q),
                    "two_queries": lambda: two_queries(e, base, cur)}
            if args.profile:
                for _ in range(args.reps):
                    arms["movers"]()
                continue
            r, t = arms["movers"](), arms["two_queries"]()  # (the warm-up: the scratch is allocated here)
            equal = bool(np.array_equal(r.services, t[0]) and np.array_equal(r.shift, t[1]) and
                         np.array_equal(r.count_base, t[2]) and np.array_equal(r.count_cur, t[3]) and
                         np.array_equal(r.q_bin_base, t[4]) and np.array_equal(r.q_bin_cur, t[5]) and r.n_matched == t[6])
            rounds = {arm: [] for arm in arms}
            for _ in range(args.rounds):
                for arm, fn in arms.items():
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn()
                    rounds[arm].append(round((time.perf_counter() - t0) / args.reps * 1e3, 4))
            med = {arm: statistics.median(v) for arm, v in rounds.items()}
            ring_bytes = 2 * length * S * 2048
            part = {"shape": name, "ring": f"{W} windows x {S} services", "range_windows": length, "spans": n,
                    "n_matched": int(r.n_matched), "ms_per_call": rounds, "median_ms": med,
                    "range_ms": {arm: [min(v), max(v)] for arm, v in rounds.items()},
                    "two_queries_over_movers": round(med["two_queries"] / med["movers"], 2),
                    "ring_bytes_read": ring_bytes, "answers_equal": equal}
            if traced:
                us = statistics.median(traced[name])
                part["sums_kernel"] = {"median_us": round(us, 2), "range_us": [round(min(traced[name]), 2), round(max(traced[name]), 2)],
                                       "dispatches": len(traced[name]), "tb_per_s": round(ring_bytes / us / 1e6, 3)}
            parts.append(part)
            print("LATENCY_MOVERS_AB " + json.dumps(part), flush=True)
    if args.profile:
        return 0
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/latency_movers_ab.py",
                   "arms": {"movers": "one window_latency_movers call, k = 10, three quantiles",
                            "two_queries": "two window_latency calls over every service and the ranking in numpy"},
                   "unit": "milliseconds of wall time per call, the mean of `reps` calls a round; sums_kernel: the "
                           "kernel's own time from a rocprofv3 --kernel-trace --stats run of the movers arm alone",
                   "rounds": args.rounds, "reps": args.reps, "parts": parts}, f, indent=1)
        f.write("\n")
    return 0 if all(p["answers_equal"] for p in parts) else 1


if __name__ == "__main__":
    sys.exit(main())
