#!/usr/bin/env python3
"""What SA_OPT_WINDOW_LATENCY costs per launch, and what sa_window_latency's
queries take -> profiles/window_latency.json.

Cost of the option.  One process holds two engines that differ only in the
option; rounds are interleaved off, on, off, on, ...; a round is `--steps`
launches of a `--spans`-span device batch, each a fresh trace-id variant
(bench.py's trace_variants), launches alternating over two streams and sa_join
before the closing event, as tools/dense_ab.py.  Shapes:

  c2         synth.generate_c2 (bench.py's C2 batch, ends drawn uniformly
             over 16 windows) in an engine of 64 services: two ring slots
             (128 KiB) of LDS histograms, one workgroup a CU, eight passes
  c2_sorted  the same spans sorted by end time, as a live stream delivers
             them: a workgroup's range lies in one window, or two
  c2_onebin  the same spans, every span of a service given one duration: all
             of a service's adds of a window land on one LDS word
  c4         synth.generate_highcard in the binned engine of bench.py's C4
             (one service: the whole 16-window ring in 16 KiB of LDS)

The record is the option's added microseconds per launch (median on minus
median off, and the rounds' ranges) against the kernel's byte floor: 20 B a
span over the measured streaming rate.  No pass or fail number is fixed.

Query time.  A ring of 1,024 windows x 32 services, loaded; the median of
`--query-reps` calls of window_latency_series at widths 1, 30 and 256 and of one
range query, against the same answers computed in numpy from one width-1
hist=True call (that call's time reported too).

Each part runs in a child process of its own under a time limit; the first
that fails ends the run.  `--worker profile` runs the c2 shape with the option
on alone, a few launches, for a kernel trace taken around it.

  python tools/latency_ab.py [--rounds 5] [--steps 10] [--spans 10000000] [--out profiles/window_latency.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))
sys.path.insert(0, ROOT)

STREAM_TBPS = 6.29  # measured HBM streaming rate of the MI355X (float4 copy)
BYTES_PER_SPAN = 20  # start_ns, end_ns, meta


def _shape(name, n):
    """(batch, first_window, engine config keywords) of a cost shape."""
    import numpy as np

    from spanagg import SpanBatch
    from spanagg.synth import generate_c2, generate_highcard

    if name == "c4":
        batch, _, first = generate_highcard(n, seed=7)
        return batch, first, dict(n_services=1, n_windows=16, key_capacity=1_200_000)
    wl = generate_c2(n, seed=42)
    batch = wl.batch
    if name == "c2_sorted":
        order = np.argsort(batch.end_ns, kind="stable")
        batch = SpanBatch(*[c[order] for c in batch.columns()])
    if name == "c2_onebin":  # one duration a service, a different bin each
        svc = (batch.meta & np.uint32(0xFFFF)).astype(np.uint64)
        dur = np.uint64(100_000) << (svc % np.uint64(16))
        batch = SpanBatch(batch.key_hash, batch.end_ns - dur, batch.end_ns, batch.trace_w0, batch.trace_w1, batch.meta)
    return batch, wl.first_window, dict(n_services=64, n_windows=16, key_capacity=1500)


def cost_worker(name, args, profile=False):
    import numpy as np
    import torch

    from bench import trace_variants
    from spanagg import Config, Engine
    from spanagg._lib import OPT_WINDOW_LATENCY

    n = args.spans
    device = torch.device("cuda", 0)
    batch, first_window, kw = _shape("c2" if profile else name, n)
    cols = [torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(device)
            for c in batch.columns()]
    arms = {"on": OPT_WINDOW_LATENCY} if profile else {"off": 0, "on": OPT_WINDOW_LATENCY}
    rounds_n, steps, warm = (1, 5, 2) if profile else (args.rounds, args.steps, args.warmup)
    variants = trace_variants(cols[3], cols[4], warm + rounds_n * steps, seed=1000)
    engines = {}
    for arm, opt in arms.items():
        e = Engine(Config(device=0, options=opt, **kw))
        e.window_advance(first_window)
        engines[arm] = e
    streams = [torch.cuda.Stream(device) for _ in range(2)]
    torch.cuda.synchronize(device)
    used = dict.fromkeys(arms, 0)

    def run(arm, k):
        e = engines[arm]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event() for _ in streams]
        torch.cuda.synchronize(device)
        a.record(streams[0])
        streams[1].wait_event(a)
        for i in range(k):
            w0, w1 = variants[used[arm] % len(variants)]
            used[arm] += 1
            e.ingest_device(cols[0], cols[1], cols[2], w0, w1, cols[5], n=n, stream=streams[i % 2].cuda_stream)
        for s, ev in zip(streams, ends):
            e.join(s.cuda_stream)
            ev.record(s)
        streams[0].wait_event(ends[1])
        b.record(streams[0])
        torch.cuda.synchronize(device)
        return a.elapsed_time(b) * 1000.0 / k

    for arm in engines:
        run(arm, warm)
    rounds = {arm: [] for arm in arms}
    for _ in range(rounds_n):
        for arm in arms:
            rounds[arm].append(round(run(arm, steps), 2))
    if profile:
        print("LATENCY_AB " + json.dumps({"shape": "profile", "us_per_launch": rounds}), flush=True)
        return 0
    # the option changes nothing else: the same RED rows and stats either way
    ra, rb = engines["off"].flush(), engines["on"].flush()
    same = bool(np.array_equal(ra.key_hash, rb.key_hash) and np.array_equal(ra.bucket_counts, rb.bucket_counts)
                and np.array_equal(ra.sum_ns, rb.sum_ns))
    lat = engines["on"].window_latency(first_window, first_window + 15)
    st = engines["on"].stats()
    counted = int(lat.count.sum()) == st["spans"] - st["invalid_service"] - st["window_out_of_range"]
    med = {arm: statistics.median(v) for arm, v in rounds.items()}
    floor_us = n * BYTES_PER_SPAN / (STREAM_TBPS * 1e12) * 1e6
    out = {"shape": name, "spans_per_launch": n, "launches_per_round": steps, "warmup_launches": warm,
           "n_services": kw["n_services"], "us_per_launch": rounds, "median_us": med,
           "min_us": {arm: min(v) for arm, v in rounds.items()}, "max_us": {arm: max(v) for arm, v in rounds.items()},
           "added_us_per_launch": round(med["on"] - med["off"], 2),
           "byte_floor_us": round(floor_us, 2), "byte_floor": f"{n * BYTES_PER_SPAN / 1e6:.0f} MB at {STREAM_TBPS} TB/s",
           "results_equal": same, "every_counted_span_in_a_histogram": counted}
    print("LATENCY_AB " + json.dumps(out), flush=True)
    return 0 if same and counted else 1


def query_worker(args):
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import latency_util as lu
    from spanagg import Config, Engine, SpanBatch, pack_meta
    from spanagg._lib import OPT_WINDOW_LATENCY

    W, S, n = 1024, 32, 4_000_000
    cfg = Config(n_services=S, n_windows=W, hll_p=8, key_capacity=1000, device=0, options=OPT_WINDOW_LATENCY)
    rng = np.random.default_rng(9)
    w0 = 1_000_000
    end = np.uint64(w0 * cfg.window_ns) + rng.integers(0, W * cfg.window_ns, n, dtype=np.uint64)
    dur = np.exp(rng.uniform(0.0, np.log(6e10), n)).astype(np.uint64)
    key = rng.integers(1, 1000, n).astype(np.uint64)
    tr = rng.integers(0, 2 ** 63, n).astype(np.uint64)
    batch = SpanBatch(key, end - dur, end, tr, tr, pack_meta(rng.integers(0, S, n), np.zeros(n), np.zeros(n)))
    q = (0.5, 0.95, 0.99)

    def timed(fn):
        t = []
        for _ in range(args.query_reps):
            t0 = time.perf_counter()
            r = fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return r, round(statistics.median(t), 3), [round(min(t), 3), round(max(t), 3)]

    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(batch)
        e.sync()
        last = w0 + W - 1
        base, base_ms, base_rng = timed(lambda: e.window_latency_series(w0, last, 1, hist=True))
        rows = []
        for width in (1, 30, 256):
            first = w0 + width - 1
            r, ms, span = timed(lambda: e.window_latency_series(first, last, width, quantiles=q))
            ref, np_ms, np_span = timed(lambda: lu.quantile_bins(lu.sliding(base.hist, width), lu.ppm_of(q)))
            equal = bool(np.array_equal(r.count, ref[0]) and np.array_equal(r.q_bin, ref[1]) and np.array_equal(r.q_ns, ref[2]))
            rows.append({"query": f"window_latency_series width {width}", "n_out": int(r.count.shape[0]),
                         "engine_ms": ms, "engine_ms_range": span, "numpy_ms": np_ms, "numpy_ms_range": np_span,
                         "equal": equal})
        r, ms, span = timed(lambda: e.window_latency(w0, last, quantiles=q))
        ref, np_ms, np_span = timed(lambda: lu.quantile_bins(base.hist.sum(axis=0, dtype=np.uint64)[None], lu.ppm_of(q)))
        equal = bool(np.array_equal(r.count, ref[0]) and np.array_equal(r.q_bin, ref[1]))
        rows.append({"query": "window_latency over the whole ring", "n_out": 1, "engine_ms": ms, "engine_ms_range": span,
                     "numpy_ms": np_ms, "numpy_ms_range": np_span, "equal": equal})
    out = {"shape": "query", "ring": f"{W} windows x {S} services", "spans": n, "reps": args.query_reps,
           "baseline": "numpy on the hist of one width-1 hist=True call (64 MiB over the bus)",
           "baseline_fetch_ms": base_ms, "baseline_fetch_ms_range": base_rng, "queries": rows}
    print("LATENCY_AB " + json.dumps(out), flush=True)
    return 0 if all(r["equal"] for r in rows) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--spans", type=int, default=10_000_000)
    ap.add_argument("--query-reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per part")
    ap.add_argument("--parts", default="c2,c2_sorted,c2_onebin,c4,query")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_latency.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "query":
        return query_worker(args)
    if args.worker:
        return cost_worker(args.worker, args, profile=args.worker == "profile")
    if args.rounds < 5:
        ap.error("at least five rounds per arm")
    results = []
    for name in args.parts.split(","):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--spans", str(args.spans), "--query-reps", str(args.query_reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("LATENCY_AB ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"latency_ab: part {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode or 1
        results.append(json.loads(line[0][len("LATENCY_AB "):]))
        print(line[0], flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/latency_ab.py",
                   "arms": {"off": "options = 0", "on": "SA_OPT_WINDOW_LATENCY"},
                   "unit": "cost shapes: microseconds per launch of spans_per_launch spans; queries: milliseconds per call",
                   "parts": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
