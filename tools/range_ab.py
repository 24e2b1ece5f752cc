#!/usr/bin/env python3
"""Engine.window_range against the path it replaces, one window_read per
window plus the numpy merge -> profiles/window_range.json.

Two geometries, one process, the product library:
  large    n_windows 1,024, hll_p 14, 32 services: a 512 MB register ring
  default  Config() with the workload's 20 services: 8 windows
Each ring is filled once (ends spread over every window, distinct traces, 5 %
ERROR spans over 700 series); 1,000 keys are queried.  Rounds are interleaved
range, loop, range, loop, ...; a round of `range` is `--calls` calls of
window_range over the full ring (the mean per call is recorded), a round of
`loop` is one pass of window_read over every window with the registers
max-merged and the cells summed in numpy.  The loop's estimates and point
queries (hll_estimate, sketch.cms_query per key) are timed apart and are not
part of the comparison: window_range's time includes its own.

The gate is relative: in every round window_range must be faster than the read
loop, on both geometries (exit status 1 otherwise).  Beside the times the file
records the bytes the merge kernel reads (the ring's registers; the cells
apart) and those bytes over the time of a whole call -- a call-level rate
that includes the fold launch, the cell sum, the queries, the copies and the
wait, so the kernel's own rate is at least that.

  python tools/range_ab.py [--rounds 5] [--calls 10] [--out profiles/window_range.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))

N_KEYS = 1000


def make_batch(rng, n, cfg, w0, pool):
    import numpy as np

    from spanagg import SpanBatch, pack_meta
    end = np.uint64(w0 * cfg.window_ns) + rng.integers(0, cfg.n_windows * cfg.window_ns, n, dtype=np.uint64)
    dur = rng.integers(1, 2_000_000_000, n, dtype=np.uint64)
    status = np.where(rng.random(n) < 0.05, 2, 0).astype(np.uint32)
    return SpanBatch(pool[rng.integers(0, len(pool), n)], end - dur, end, rng.integers(0, 2**64, n, dtype=np.uint64),
                     rng.integers(0, 2**64, n, dtype=np.uint64),
                     pack_meta(rng.integers(0, cfg.n_services, n), rng.integers(0, 6, n), status))


def read_loop(e, w0, W):
    """The replaced path: every window read to the host, merged in numpy."""
    import numpy as np
    hll = cms = None
    for w in range(w0, w0 + W):
        sk = e.window_read(w)
        hll = sk.hll if hll is None else np.maximum(hll, sk.hll, out=hll)
        cms = sk.cms.astype(np.uint64) if cms is None else cms + sk.cms
    return hll, cms


def measure(name, cfg, spans, args):
    import numpy as np

    from spanagg import Engine, hll_estimate
    from spanagg.sketch import cms_query
    rng = np.random.default_rng(11)
    pool = rng.integers(1, 2**64, 700, dtype=np.uint64)
    keys = np.concatenate([pool, rng.integers(1, 2**64, N_KEYS - len(pool), dtype=np.uint64)])
    w0, W = 176_722_560, cfg.n_windows
    with Engine(cfg) as e:
        e.window_advance(w0)
        for _ in range(spans // 1_000_000):
            e.ingest(make_batch(rng, 1_000_000, cfg, w0, pool))
        e.sync()
        r = e.window_range(w0, w0 + W - 1, keys)  # warm both arms, and the two must agree
        hll, cms = read_loop(e, w0, W)
        same = bool(np.array_equal(r.hist, np.stack([np.bincount(row, minlength=64) for row in hll]))
                    and [int(x) for x in r.errors] == [cms_query(cms, int(k)) for k in keys])
        rounds = {"range_us_per_call": [], "loop_us": [], "loop_estimates_and_queries_us": []}
        for _ in range(args.rounds):
            t = time.perf_counter()
            for _ in range(args.calls):
                e.window_range(w0, w0 + W - 1, keys)  # (returns after its own wait on the engine stream)
            rounds["range_us_per_call"].append(round((time.perf_counter() - t) * 1e6 / args.calls, 1))
            t = time.perf_counter()
            hll, cms = read_loop(e, w0, W)
            rounds["loop_us"].append(round((time.perf_counter() - t) * 1e6, 1))
            t = time.perf_counter()
            [hll_estimate(row, cfg.hll_p) for row in hll], [cms_query(cms, int(k)) for k in keys]
            rounds["loop_estimates_and_queries_us"].append(round((time.perf_counter() - t) * 1e6, 1))
    reg_bytes = (W * cfg.n_services) << cfg.hll_p
    med = statistics.median(rounds["range_us_per_call"])
    return {"geometry": name, "n_windows": W, "n_services": cfg.n_services, "hll_p": cfg.hll_p, "spans": spans,
            "n_keys": N_KEYS, "calls_per_range_round": args.calls, **rounds,
            "median_range_us_per_call": med, "median_loop_us": statistics.median(rounds["loop_us"]),
            "merge_kernel_register_bytes": reg_bytes, "cell_sum_bytes": W * cfg.cms_d * cfg.cms_w * 8,
            "loop_bytes_over_pcie": reg_bytes + W * cfg.cms_d * cfg.cms_w * 8,
            "register_gb_per_s_over_call_time": round(reg_bytes / med / 1e3, 1),
            "range_faster_every_round": all(a < b for a, b in zip(rounds["range_us_per_call"], rounds["loop_us"])),
            "results_equal": same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_range.json"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds")
    from spanagg import Config
    out = [measure("large", Config(n_windows=1024, hll_p=14, n_services=32), 4_000_000, args),
           measure("default", Config(n_services=20), 2_000_000, args)]
    for g in out:
        print("RANGE_AB " + json.dumps(g), flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/range_ab.py", "unit": "microseconds (host clock around calls that end in a wait)",
                   "arms": {"range": "Engine.window_range over the full ring, 1,000 keys",
                            "loop": "Engine.window_read per window + numpy maximum / sum"},
                   "geometries": out}, f, indent=1)
        f.write("\n")
    return 0 if all(g["range_faster_every_round"] and g["results_equal"] for g in out) else 1


if __name__ == "__main__":
    sys.exit(main())
