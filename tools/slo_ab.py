#!/usr/bin/env python3
"""What sa_window_slo takes against the only way to the same answers without
it -> profiles/window_slo.json.

The ring is 1,024 windows x 32 services holding 4 M spans (the shape DESIGN.md
uses for the latency queries).  The query: window_slo with widths (6, 30, 180,
360) over every output they allow (665), every service, a threshold a service.
The record is the median and range of `--reps` calls.

The baseline is what a caller of the parent library does: one width-1
hist=True window_latency_series call over the whole ring (64 MiB over the bus)
and the same total, slow and burning computed from its histograms in numpy.
The call's time and numpy's are reported apart; the answers must be equal.

Stage 1 (slo_pairs_kernel) reads n_cov x n_sel x 2 KiB of the ring once.  Its
own time comes from a kernel trace: `--worker profile` makes `--reps` calls
alone, for a rocprofv3 --kernel-trace run around it, and `--kernel-trace CSV`
adds both kernels' medians, stage 1's bytes over its time, and its share of
the call, beside the measured streaming rate of the MI355X.

Each part runs in a child process of its own under a time limit; the first
that fails ends the run.

  python tools/slo_ab.py [--reps 5] [--kernel-trace CSV] [--out profiles/window_slo.json]
"""
import argparse
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))
sys.path.insert(0, ROOT)

STREAM_TBPS = 6.29  # measured HBM streaming rate of the MI355X (float4 copy), as tools/latency_ab.py quotes it
W, S, N = 1024, 32, 4_000_000
WIDTHS, LIMITS, MIN_COUNT = (6, 30, 180, 360), (144_000, 60_000, 30_000, 10_000), 100
KERNELS = ("slo_pairs_kernel", "slo_slide_kernel")


def load():
    """The loaded engine, its first window and a threshold a service."""
    import numpy as np

    from spanagg import Config, Engine, SpanBatch, pack_meta
    from spanagg._lib import OPT_WINDOW_LATENCY

    cfg = Config(n_services=S, n_windows=W, hll_p=8, key_capacity=1000, device=0, options=OPT_WINDOW_LATENCY)
    rng = np.random.default_rng(9)
    w0 = 1_000_000
    end = np.uint64(w0 * cfg.window_ns) + rng.integers(0, W * cfg.window_ns, N, dtype=np.uint64)
    dur = np.exp(rng.uniform(0.0, np.log(6e10), N)).astype(np.uint64)
    key = rng.integers(1, 1000, N).astype(np.uint64)
    tr = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = Engine(cfg)
    e.window_advance(w0)
    e.ingest(SpanBatch(key, end - dur, end, tr, tr, pack_meta(rng.integers(0, S, N), np.zeros(N), np.zeros(N))))
    e.sync()
    thresholds = np.exp(rng.uniform(np.log(1e8), np.log(2e10), S)).astype(np.uint64)  # 0.1 s .. 20 s
    return e, w0, thresholds


def from_histograms(hist, thresholds):
    """total, slow [n_out][n_widths][S] and burning [n_out][S] from the width-1
    histograms [W][S][256] of the whole ring, in numpy."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import latency_util as lu

    mw = max(WIDTHS)
    above = np.arange(256)[None, :] > lu.bins_of(thresholds)[:, None]
    tot = hist.sum(axis=-1, dtype=np.uint64)
    slo = np.where(above[None], hist, np.uint64(0)).sum(axis=-1, dtype=np.uint64)
    total = np.stack([lu.sliding(tot, w)[mw - w:] for w in WIDTHS], axis=1)
    slow = np.stack([lu.sliding(slo, w)[mw - w:] for w in WIDTHS], axis=1)
    burns = (total >= np.uint64(MIN_COUNT)) & \
        (slow * np.uint64(1_000_000) > np.asarray(LIMITS, dtype=np.uint64)[None, :, None] * total)
    burning = np.zeros(burns.shape[::2], np.uint8)
    for w in range(len(WIDTHS)):
        burning |= burns[:, w].astype(np.uint8) << np.uint8(w)
    return total, slow, burning


def query_worker(args):
    import numpy as np

    def timed(fn):
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fn()
            t.append((time.perf_counter() - t0) * 1e3)
        return r, round(statistics.median(t), 3), [round(min(t), 3), round(max(t), 3)]

    e, w0, thresholds = load()
    with e:
        first, last = w0 + max(WIDTHS) - 1, w0 + W - 1
        slo = lambda: e.window_slo(first, last, WIDTHS, LIMITS, thresholds, min_count=MIN_COUNT)
        slo()  # (the warm-up: the scratch is allocated here)
        r, ms, span = timed(slo)
        base, base_ms, base_span = timed(lambda: e.window_latency_series(w0, last, 1, hist=True))
        ref, np_ms, np_span = timed(lambda: from_histograms(base.hist, thresholds))
    equal = bool(np.array_equal(r.total, ref[0]) and np.array_equal(r.slow, ref[1]) and np.array_equal(r.burning, ref[2]))
    n_out, n_cov = int(r.total.shape[0]), int(r.total.shape[0]) + max(WIDTHS) - 1
    out = {"part": "query", "ring": f"{W} windows x {S} services", "spans": N, "reps": args.reps,
           "widths": list(WIDTHS), "limit_ppm": list(LIMITS), "min_count": MIN_COUNT, "n_out": n_out, "n_cov": n_cov,
           "window_slo_ms": ms, "window_slo_ms_range": span,
           "baseline": "one width-1 hist=True window_latency_series call over the ring, then numpy",
           "baseline_call_ms": base_ms, "baseline_call_ms_range": base_span,
           "baseline_numpy_ms": np_ms, "baseline_numpy_ms_range": np_span,
           "baseline_over_window_slo": round((base_ms + np_ms) / ms, 1),
           "bus_bytes": {"window_slo": int(r.total.nbytes + r.slow.nbytes + r.burning.nbytes + r.alert_outputs.nbytes),
                         "baseline": int(base.hist.nbytes + base.count.nbytes + base.q_bin.nbytes)},
           "stage1_ring_bytes_read": n_cov * S * 2048,
           "rows_burning": int((r.burning != 0).sum()), "alert_outputs": int(r.alert_outputs.sum()),
           "answers_equal": equal}
    print("SLO_AB " + json.dumps(out), flush=True)
    return 0 if equal else 1


def profile_worker(args):
    e, w0, thresholds = load()
    with e:
        for _ in range(args.reps):
            e.window_slo(w0 + max(WIDTHS) - 1, w0 + W - 1, WIDTHS, LIMITS, thresholds, min_count=MIN_COUNT)
    return 0


def kernel_times(path, reps):
    """{kernel: its dispatches' us} from a rocprofv3 kernel-trace CSV of a --worker profile run."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {}
    for k in KERNELS:
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
        if len(us) != reps:
            raise SystemExit(f"{path}: {len(us)} dispatches of {k}, expected {reps}")
        out[k] = us
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per part")
    ap.add_argument("--kernel-trace", default=None, help="the kernel-trace CSV of a --worker profile run with the same --reps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_slo.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker == "query":
        return query_worker(args)
    if args.worker == "profile":
        return profile_worker(args)
    if args.reps < 5:
        ap.error("at least five calls")
    traced = kernel_times(args.kernel_trace, args.reps) if args.kernel_trace else None
    results = []
    for name in ("query",):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("SLO_AB ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"slo_ab: part {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode or 1
        results.append(json.loads(line[0][len("SLO_AB "):]))
        print(line[0], flush=True)
    q = results[0]
    if traced:
        med = {k: statistics.median(v) for k, v in traced.items()}
        q["kernels"] = {k: {"median_us": round(med[k], 2), "range_us": [round(min(v), 2), round(max(v), 2)],
                            "dispatches": len(v)} for k, v in traced.items()}
        q["stage1"] = {"ring_bytes_read": q["stage1_ring_bytes_read"], "median_us": round(med[KERNELS[0]], 2),
                       "tb_per_s": round(q["stage1_ring_bytes_read"] / med[KERNELS[0]] / 1e6, 3),
                       "streaming_tb_per_s": STREAM_TBPS,
                       "share_of_the_call": round(med[KERNELS[0]] / 1e3 / q["window_slo_ms"], 3)}
    else:
        q["kernels"] = "not measured: no --kernel-trace given"
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/slo_ab.py",
                   "unit": "milliseconds of wall time per call; kernels: microseconds of the kernel's own time from a "
                           "rocprofv3 --kernel-trace run of --worker profile",
                   "parts": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
