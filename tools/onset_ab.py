#!/usr/bin/env python3
"""What sa_window_latency_onset takes against the only way to the same answer
without it -> profiles/window_onset.json.

The ring is 1,024 windows x 256 services (the largest ring sa_create allows)
holding 4 M spans; every fourth service's durations are multiplied by 6 from a
drawn window on.  The query: window_latency_onset over the whole ring, k = 10,
min_count 100, under the pooled threshold (quantile 0.95) and under given
thresholds (one a service).

The baseline is what a caller of the parent library does for the given
thresholds: one window_slo call at width 1 over every window and service (the
(total, slow) pairs, 4 MiB over the bus twice) and the change-point scan, the
match rule and the order in numpy -- in int64, which is exact here because a
service holds far fewer than 2^31 spans; counts near 2^43 would need Python
integers.  (For the pooled threshold the baseline would also need a
window_latency call of width 1,024 for the quantile bins; its time is reported
apart.)  The call's time and numpy's are reported apart; the answers must be
equal.

The three are timed in turn, rep after rep, after `--warmup` rounds: wall time
around each call, which ends in the call's one wait for the engine stream.  The
worker runs in a child process of its own under a time limit.

  python tools/onset_ab.py [--reps 20] [--warmup 3] [--out profiles/window_onset.json]
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

W, S, N = 1024, 256, 4_000_000
K, MIN_COUNT, QUANTILE = 10, 100, 0.95


def load():
    """The loaded engine, its first window and a threshold a service."""
    import numpy as np

    from spanagg import Config, Engine, SpanBatch, pack_meta
    from spanagg._lib import OPT_WINDOW_LATENCY

    cfg = Config(n_services=S, n_windows=W, hll_p=8, key_capacity=1000, device=0, options=OPT_WINDOW_LATENCY)
    rng = np.random.default_rng(11)
    w0 = 1_000_000
    end = np.uint64(w0 * cfg.window_ns) + rng.integers(0, W * cfg.window_ns, N, dtype=np.uint64)
    svc = rng.integers(0, S, N)
    dur = np.exp(rng.uniform(np.log(1e5), np.log(1e9), N))
    at = rng.integers(1, W, S)  # the window a shifted service's change begins at
    win = (end // np.uint64(cfg.window_ns)).astype(np.int64) - w0
    dur[(svc % 4 == 0) & (win >= at[svc])] *= 6.0
    dur = dur.astype(np.uint64)
    key = rng.integers(1, 1000, N).astype(np.uint64)
    tr = rng.integers(0, 2 ** 63, N).astype(np.uint64)
    e = Engine(cfg)
    e.window_advance(w0)
    e.ingest(SpanBatch(key, end - dur, end, tr, tr, pack_meta(svc, np.zeros(N), np.zeros(N))))
    e.sync()
    thresholds = np.exp(rng.uniform(np.log(1e8), np.log(6e8), S)).astype(np.uint64)  # 0.1 s .. 0.6 s
    return e, w0, thresholds


def scan_in_numpy(total, slow, k, min_count):
    """sa_window_latency_onset's rule on (total, slow) [n_cov][S] of every window
    and service, in int64: (services, onset index, delta_ppm, n_eligible,
    n_matched) of the first k."""
    import numpy as np

    tot, slo = total.astype(np.int64), slow.astype(np.int64)
    nb, sb = np.cumsum(tot, axis=0)[:-1], np.cumsum(slo, axis=0)[:-1]  # split t = row + 1
    n, s = tot.sum(axis=0), slo.sum(axis=0)
    na, sa = n[None] - nb, s[None] - sb
    elig = (nb >= min_count) & (na >= min_count)
    d = np.where(elig, sa * nb - sb * na, np.iinfo(np.int64).min)
    rows = d.shape[0]
    best = rows - 1 - np.argmax(d[::-1], axis=0)  # the latest among equal D
    has = elig.any(axis=0)
    col = np.arange(tot.shape[1])
    bnb, bsb, bna, bsa = nb[best, col], sb[best, col], na[best, col], sa[best, col]
    delta = np.where(has, bsa * 1_000_000 // np.maximum(bna, 1) - bsb * 1_000_000 // np.maximum(bnb, 1), 0)
    match = has & (d[best, col] > 0) & (delta >= 1)
    ids = np.flatnonzero(match)
    order = ids[np.lexsort((ids, -np.minimum(n[ids], (1 << 44) - 1), -delta[ids]))][:k]
    return order, best[order] + 1, delta[order], int(has.sum()), int(match.sum())


def worker(args):
    import numpy as np

    e, w0, thresholds = load()
    first, last = w0, w0 + W - 1
    with e:
        pooled = lambda: e.window_latency_onset(first, last, K, QUANTILE, None, MIN_COUNT)
        given = lambda: e.window_latency_onset(first, last, K, 0.0, thresholds, MIN_COUNT)
        slo = lambda: e.window_slo(first, last, (1,), (0,), thresholds)
        quant = lambda: e.window_latency_series(last, last, W, quantiles=(QUANTILE,))
        parts = {"pooled": pooled, "given": given, "baseline_call": slo, "baseline_quantile_call": quant}
        for _ in range(args.warmup):  # (the scratch is allocated here, the code objects loaded)
            for fn in parts.values():
                fn()
        ms, res = {name: [] for name in parts}, {}
        ms["baseline_numpy"] = []
        for _ in range(args.reps):
            for name, fn in parts.items():
                t0 = time.perf_counter()
                res[name] = fn()
                ms[name].append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter()
            b = res["baseline_call"]
            ref = scan_in_numpy(b.total[:, 0], b.slow[:, 0], K, MIN_COUNT)
            ms["baseline_numpy"].append((time.perf_counter() - t0) * 1e3)
    g = res["given"]
    equal = bool(np.array_equal(g.services, ref[0]) and np.array_equal(g.onset_window, ref[1] + w0) and
                 np.array_equal(g.delta_ppm, ref[2]) and (g.n_eligible, g.n_matched) == ref[3:])
    stat = lambda v: {"median_ms": round(statistics.median(v), 3), "range_ms": [round(min(v), 3), round(max(v), 3)]}
    p = res["pooled"]
    out = {"ring": f"{W} windows x {S} services", "spans": N, "reps": args.reps, "warmup": args.warmup, "k": K,
           "min_count": MIN_COUNT, "quantile": QUANTILE,
           "clock": "host wall time around the call; every call ends in its one wait for the engine stream",
           "window_latency_onset_pooled": stat(ms["pooled"]), "window_latency_onset_given": stat(ms["given"]),
           "baseline": "window_slo at width 1 over every window and service, then the scan in numpy (int64)",
           "baseline_call": stat(ms["baseline_call"]), "baseline_numpy": stat(ms["baseline_numpy"]),
           "baseline_quantile_call": stat(ms["baseline_quantile_call"]),
           "baseline_over_given": round((statistics.median(ms["baseline_call"]) + statistics.median(ms["baseline_numpy"])) /
                                        statistics.median(ms["given"]), 1),
           "given": {"n_eligible": g.n_eligible, "n_matched": g.n_matched, "rows": g.items()[:3]},
           "pooled": {"n_eligible": p.n_eligible, "n_matched": p.n_matched, "rows": p.items()[:3]},
           "answers_equal": equal}
    print("ONSET_AB " + json.dumps(out), flush=True)
    return 0 if equal else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the worker")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_onset.json"))
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    if args.reps < 5:
        ap.error("at least five calls")
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker",
           "--reps", str(args.reps), "--warmup", str(args.warmup)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in p.stdout.splitlines() if l.startswith("ONSET_AB ")]
    if not line:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        print(f"onset_ab: the worker failed (exit {p.returncode})", file=sys.stderr)
        return p.returncode or 1
    print(line[0], flush=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/onset_ab.py", "unit": "milliseconds of wall time per call",
                   "result": json.loads(line[0][len("ONSET_AB "):])}, f, indent=1)
        f.write("\n")
    return p.returncode


if __name__ == "__main__":
    sys.exit(main())
