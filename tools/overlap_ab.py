#!/usr/bin/env python3
"""Engine.window_overlap against what a caller does without it:
window_range(registers=True), then on the host the pairwise np.maximum,
np.bincount and hll_estimate_hist -> profiles/window_overlap.json.

Two shapes, one process:
  default   Config(): 64 services, hll_p 14, 8 windows; all 2,016 pairs
  ring1024  the 1,024-window ring of tools/range_ab.py: hll_p 14, 32 services;
            all 496 pairs over the full ring
Each ring is filled once: a trace visits a run of 1..8 consecutive services and
its spans end anywhere in the ring, so the pairs overlap by graded amounts.
Rounds are interleaved overlap, host, overlap, host, ...: a round of `overlap`
is `--calls` calls of window_overlap over the full ring (the mean per call is
recorded), a round of `host` is one window_range(registers=True) and the numpy
pairs.  Both legs end with the same numbers on the host (compared once,
exactly), and both end in the engine's own wait, so the host clock around them
measures whole calls.  The file records every round, the median and the range
per leg, and whether the device call was below the host way in every round;
nothing is gated on the times.

A third engine (hll_p 18, 64 services, 2 windows) times window_overlap alone:
2,016 pairs of 2^18 registers, the pair kernel's largest job.

With the laboratory library (SPANAGG_LIB=.../libspanagg_ab.so) the tool also
interleaves the pair kernel's counting variants (SPANAGG_OVERLAP=0, 1, 2, read
at every call) on the default and the hll_p 18 engines: the calls differ in
that kernel alone, so the differences between the legs are the kernel's.

  python tools/overlap_ab.py [--rounds 5] [--calls 10] [--out profiles/window_overlap.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))

W0 = 176_722_560
VARIANTS = {"0": "lanes are the tile's 64 pairs, a private LDS row each (the product's)",
            "1": "lanes are columns, 16 words in registers, one LDS add a register",
            "2": "as 1, the values 0..3 by ballot and popcount"}


def legs(rounds):
    return {name: {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)} for name, v in rounds.items()}


def make_batch(rng, n_runs, cfg):
    """n_runs traces, each on a run of 1..8 consecutive services, one span a visit."""
    import numpy as np

    from spanagg import SpanBatch, pack_meta
    length = rng.integers(1, 9, n_runs)
    start = rng.integers(0, cfg.n_services, n_runs)
    tr = np.repeat(np.arange(n_runs), length)
    svc = np.repeat(start, length) + np.concatenate([np.arange(k) for k in length])
    keep = svc < cfg.n_services
    tr, svc = tr[keep], svc[keep]
    n = len(tr)
    t0, t1 = rng.integers(0, 2**64, n_runs, dtype=np.uint64), rng.integers(0, 2**64, n_runs, dtype=np.uint64)
    end = np.uint64(W0 * cfg.window_ns) + rng.integers(0, cfg.n_windows * cfg.window_ns, n, dtype=np.uint64)
    pool = rng.integers(1, 2**64, 700, dtype=np.uint64)
    return SpanBatch(pool[rng.integers(0, len(pool), n)], end - rng.integers(1, 2_000_000_000, n, dtype=np.uint64), end,
                     t0[tr], t1[tr], pack_meta(svc, rng.integers(0, 6, n), np.zeros(n, np.uint32)))


def host_way(e, first, last, p):
    """The parent commit's API: the merged registers over the bus, the pairs in numpy."""
    import numpy as np

    from spanagg import hll_estimate_hist
    r = e.window_range(first, last, registers=True)
    n = len(r.hll)
    shared = np.diag(r.distinct)
    for i in range(n):
        for j in range(i + 1, n):
            u = hll_estimate_hist(np.bincount(np.maximum(r.hll[i], r.hll[j]), minlength=64), p)
            shared[i, j] = shared[j, i] = max(0.0, (r.distinct[i] + r.distinct[j]) - u)
    return shared


def loaded(cfg, n_runs, seed):
    import numpy as np

    from spanagg import Engine
    e = Engine(cfg)
    e.window_advance(W0)
    b = make_batch(np.random.default_rng(seed), n_runs, cfg)
    for a in range(0, len(b), 1_000_000):
        e.ingest(b.slice(a, min(len(b), a + 1_000_000)))
    e.sync()
    return e, len(b)


def timed_calls(e, first, last, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        e.window_overlap(first, last)
    return round((time.perf_counter() - t0) * 1e6 / calls, 1)


def measure(name, cfg, n_runs, args):
    import numpy as np
    first, last = W0, W0 + cfg.n_windows - 1
    e, spans = loaded(cfg, n_runs, 11)
    with e:
        r = e.window_overlap(first, last)  # warm both legs, and the two must agree
        same = np.array_equal(r.shared, host_way(e, first, last, cfg.hll_p))
        rounds = {"overlap_us_per_call": [], "range_then_host_pairs_us": []}
        for _ in range(args.rounds):
            rounds["overlap_us_per_call"].append(timed_calls(e, first, last, args.calls))
            t0 = time.perf_counter()
            host_way(e, first, last, cfg.hll_p)
            rounds["range_then_host_pairs_us"].append(round((time.perf_counter() - t0) * 1e6, 1))
    n = cfg.n_services
    return {"shape": name, "n_windows": cfg.n_windows, "n_services": n, "hll_p": cfg.hll_p, "spans": spans,
            "pairs": n * (n - 1) // 2, "register_bytes_over_the_bus_host_way": n << cfg.hll_p,
            "histogram_bytes_over_the_bus_overlap": (n + n * (n - 1) // 2) * 64 * 4,
            "largest_shared": float(np.triu(r.shared, 1).max()), "calls_per_overlap_round": args.calls, **rounds,
            "legs": legs(rounds),
            "overlap_below_host_every_round": all(a < b for a, b in zip(rounds["overlap_us_per_call"],
                                                                        rounds["range_then_host_pairs_us"])),
            "results_equal": bool(same)}


def kernel_only(cfg, n_runs, args, lab):
    """window_overlap alone at hll_p 18 (and per counting variant with the laboratory library)."""
    first, last = W0, W0 + cfg.n_windows - 1
    e, spans = loaded(cfg, n_runs, 13)
    names = list(VARIANTS) if lab else ["0"]
    with e:
        ref = e.window_overlap(first, last)
        rounds = {v: [] for v in names}
        equal = True
        for _ in range(args.rounds):
            for v in names:
                if lab:
                    os.environ["SPANAGG_OVERLAP"] = v
                rounds[v].append(timed_calls(e, first, last, args.calls))
                equal = equal and bool((e.window_overlap(first, last).pair_hist == ref.pair_hist).all())
        os.environ.pop("SPANAGG_OVERLAP", None)
    n = cfg.n_services
    return {"n_windows": cfg.n_windows, "n_services": n, "hll_p": cfg.hll_p, "spans": spans, "pairs": n * (n - 1) // 2,
            "registers_a_pair": 1 << cfg.hll_p, "overlap_us_per_call_by_variant": rounds, "legs": legs(rounds),
            "variants_equal": equal}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_overlap.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds")
    from spanagg import Config
    lab = "libspanagg_ab" in (os.environ.get("SPANAGG_LIB") or "")
    doc = {"tool": "tools/overlap_ab.py", "library": "laboratory" if lab else "product",
           "unit": "microseconds (host clock around calls that end in a wait)",
           "legs": {"overlap": "Engine.window_overlap(first, last) over the full ring, every pair",
                    "range_then_host_pairs": "Engine.window_range(first, last, registers=True) + numpy maximum, "
                                             "bincount and hll_estimate_hist per pair"}}
    if lab:
        doc["variants"] = VARIANTS
        doc["variant_ab"] = [kernel_only(Config(), 200_000, args, True),
                             kernel_only(Config(hll_p=18, n_windows=2), 600_000, args, True)]
        ok = all(g["variants_equal"] for g in doc["variant_ab"])
    else:
        doc["shapes"] = [measure("default", Config(), 200_000, args),
                         measure("ring1024", Config(n_windows=1024, hll_p=14, n_services=32), 900_000, args)]
        doc["p18_call_alone"] = kernel_only(Config(hll_p=18, n_windows=2), 600_000, args, False)
        ok = all(g["results_equal"] for g in doc["shapes"])
    print("OVERLAP_AB " + json.dumps(doc), flush=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
