#!/usr/bin/env python3
"""A/B of the default binned path against dense series indices
(SA_OPT_DENSE_IDS) on bench.py's C4 workloads -> profiles/dense_ab.json.

For `c4` (uniform) and `c4zipf` (Zipf 1.1) -- bench.py's generator, sizes,
fresh trace-id variant per launch, launches alternating over two streams and
sa_join before the closing event -- one process holds both engines: A, the
default engine fed the series hashes, and B, a dense engine fed the indices
of a DenseIds dictionary (all bound before the first launch, as a host whose
series are known would).  Rounds are interleaved A, B, A, B, ...; a round is
`--steps` launches and reports microseconds per launch.  Each workload runs in
a child process of its own under a time limit; the first that fails ends the
run.

The dense path is called faster only when every dense round beats every
binned round of the same workload; otherwise the medians and the spread are
what there is to say.

  python tools/dense_ab.py [--rounds 6] [--steps 20] [--spans 10000000] [--out profiles/dense_ab.json]
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


def worker(name, args):
    import numpy as np
    import torch

    from bench import trace_variants
    from spanagg import Config, Engine
    from spanagg._lib import OPT_DENSE_IDS
    from spanagg.synth import generate_highcard

    n = args.spans
    device = torch.device("cuda", 0)
    batch, _, first_window = generate_highcard(n, seed=7, zipf_s=1.1 if name == "c4zipf" else 0.0)
    cols = [torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(device)
            for c in batch.columns()]
    warm = args.warmup
    per_arm = warm + args.rounds * args.steps
    # both engines see the same sequence of variants, each of them once
    variants = trace_variants(cols[3], cols[4], per_arm, seed=1000)
    engines = {}
    for arm, opt in (("binned", 0), ("dense", OPT_DENSE_IDS)):
        e = Engine(Config(n_services=1, n_windows=16, key_capacity=1_200_000, device=0, options=opt))
        e.window_advance(first_window)
        engines[arm] = e
    t0 = time.perf_counter()
    ids, new_i, new_h = engines["dense"].ids.encode(batch.key_hash)
    encode_s = time.perf_counter() - t0
    engines["dense"].bind_ids(new_i, new_h)
    keys = {"binned": cols[0], "dense": torch.from_numpy(ids.view(np.int64)).to(device)}
    streams = [torch.cuda.Stream(device) for _ in range(2)]
    torch.cuda.synchronize(device)
    used = {"binned": 0, "dense": 0}

    def run(arm, steps):
        e = engines[arm]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ends = [torch.cuda.Event() for _ in streams]
        torch.cuda.synchronize(device)
        a.record(streams[0])
        streams[1].wait_event(a)
        for i in range(steps):
            w0, w1 = variants[used[arm] % len(variants)]
            used[arm] += 1
            e.ingest_device(keys[arm], cols[1], cols[2], w0, w1, cols[5], n=n, stream=streams[i % 2].cuda_stream)
        for s, ev in zip(streams, ends):
            e.join(s.cuda_stream)
            ev.record(s)
        streams[0].wait_event(ends[1])
        b.record(streams[0])
        torch.cuda.synchronize(device)
        return a.elapsed_time(b) * 1000.0 / steps

    for arm in engines:
        run(arm, warm)
    rounds = {"binned": [], "dense": []}
    for _ in range(args.rounds):
        for arm in ("binned", "dense"):
            rounds[arm].append(round(run(arm, args.steps), 2))
    # the two engines computed the same thing
    ra, rb = engines["binned"].flush(), engines["dense"].flush()
    same = bool(np.array_equal(ra.key_hash, rb.key_hash) and np.array_equal(ra.bucket_counts, rb.bucket_counts)
                and np.array_equal(ra.sum_ns, rb.sum_ns))
    dropped = {arm: e.stats()["dropped_table_full"] for arm, e in engines.items()}
    out = {"workload": name, "spans_per_step": n, "steps_per_round": args.steps, "warmup_steps": warm,
           "us_per_step": rounds,
           "median_us": {arm: statistics.median(v) for arm, v in rounds.items()},
           "min_us": {arm: min(v) for arm, v in rounds.items()},
           "max_us": {arm: max(v) for arm, v in rounds.items()},
           "dense_faster_every_round": max(rounds["dense"]) < min(rounds["binned"]),
           "results_equal": same, "dropped_table_full": dropped, "series": int(len(ra.key_hash)),
           "host_encode_s": round(encode_s, 3)}
    print("DENSE_AB " + json.dumps(out), flush=True)
    return 0 if same and not any(dropped.values()) else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--spans", type=int, default=10_000_000)
    ap.add_argument("--timeout", type=int, default=280, help="seconds per workload")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_ab.json"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("at least five rounds per arm")
    if args.worker:
        return worker(args.worker, args)
    results = []
    for name in ("c4", "c4zipf"):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--worker", name,
               "--rounds", str(args.rounds), "--steps", str(args.steps), "--warmup", str(args.warmup),
               "--spans", str(args.spans)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in p.stdout.splitlines() if l.startswith("DENSE_AB ")]
        if p.returncode != 0 or not line:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            print(f"dense_ab: workload {name} failed (exit {p.returncode}); stopping", file=sys.stderr)
            return p.returncode or 1
        results.append(json.loads(line[0][len("DENSE_AB "):]))
        print(line[0])
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/dense_ab.py", "unit": "microseconds per launch of spans_per_step spans",
                   "arms": {"binned": "default engine, series hashes", "dense": "SA_OPT_DENSE_IDS, dense indices"},
                   "workloads": results}, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
