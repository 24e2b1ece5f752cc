#!/usr/bin/env python3
"""Times Engine.window_error_onset (k = 10) against the host route a caller had
before it: one window_range(w, w, cells=True) per window of the range, the
prefix sums, the resident keys hashed into every row and the split scan in
numpy (tests/error_onset_util.onset) -- in one process, five interleaved
rounds, host clock around calls that end in their own device wait.  The two
answers are asserted equal before anything is timed.  DESIGN.md section 4,
"Error onset over the window ring".

  default   synth.generate_c2 (1,500 series) on the default engine, 8 windows
  ring1024  the same series spread over a ring of 1,024 windows (hll_p 4, so
            the ring stays small; the default 4 x 2,048 count-min)
  c4        synth.generate_highcard (1,000,000 series, key_capacity 1,200,000,
            16 windows, count-min 4 x 65,536)

--device-only leaves the host route out (a run under a kernel trace of its
own); --check-only runs it once for the assertion and does not time it.
--label names the library measured: SPANAGG_LIB selects another build, and on
the laboratory build SPANAGG_EO_WAVE=1 the scan with a wave a candidate (the
lane-mapping A/B; the two runs' files are compared by hand).  One JSON line
per engine, and --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "opentelemetry-demo_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]

ROUNDS = 5


def host_route(e, first, last, cand, k):
    import error_onset_util as eu
    windows = {w: (None, e.window_range(w, w, cells=True).cms) for w in range(first, last + 1)}
    return eu.onset(windows, first, last, cand, k)


def timed(e, first, last, cand, reps_dev, reps_host, check):
    import error_onset_util as eu
    r = e.window_error_onset(first, last, 10)
    same = None
    if check:
        want = host_route(e, first, last, cand, 10)
        eu.assert_onset_equal(r, want, "device call against the host route")
        same = True
    dev, host = [], []
    for _ in range(ROUNDS):
        t = []
        for _ in range(reps_dev):
            t0 = time.perf_counter()
            e.window_error_onset(first, last, 10)
            t.append(time.perf_counter() - t0)
        dev.append(statistics.median(t))
        t = []
        for _ in range(reps_host):
            t0 = time.perf_counter()
            host_route(e, first, last, cand, 10)
            t.append(time.perf_counter() - t0)
        if t:
            host.append(statistics.median(t))
    q = lambda v: [round(1e6 * x, 1) for x in (statistics.median(v), min(v), max(v))] if v else None
    return dict(device_us=q(dev), host_route_us=q(host), answers_equal=same, n_resident=r.n_resident,
                n_eligible=r.n_eligible, n_matched=r.n_matched, calls_a_round=[reps_dev, reps_host])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="product")
    ap.add_argument("--engines", default="default,ring1024,c4")
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--check-only", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import numpy as np

    from spanagg import Config, Engine
    from spanagg.synth import generate_c2, generate_highcard
    legs = []
    for name in args.engines.split(","):
        if name == "default":
            wl = generate_c2(400_003, seed=21)
            cfg, w0, batch, reps = Config(n_services=wl.n_services, n_windows=8), wl.first_window, wl.batch, (100, 20)
        elif name == "ring1024":
            wl = generate_c2(400_003, seed=21, spread_s=10_200)
            cfg, w0, batch = Config(n_services=wl.n_services, n_windows=1024, hll_p=4), wl.first_window, wl.batch
            reps = (40, 3)
        elif name == "c4":
            batch, _, w0 = generate_highcard(4_000_000, seed=7)
            cfg, reps = Config(n_services=1, n_windows=16, key_capacity=1_200_000, cms_d=4, cms_w=65536), (20, 1)
        else:
            ap.error(f"unknown engine {name}")
        first, last = w0, w0 + cfg.n_windows - 1
        with Engine(cfg) as e:
            e.window_advance(w0)
            e.ingest(batch)
            cand = np.unique(batch.key_hash)  # the caller's own list of its series: what the key table holds
            cand = cand[cand != 0]
            assert len(cand) == e.stats()["n_keys"], (len(cand), e.stats()["n_keys"])
            leg = dict(engine=name, lib=args.label, cells=[cfg.cms_d, cfg.cms_w], windows=cfg.n_windows,
                       slots=e.stats()["table_capacity"],
                       wave=os.environ.get("SPANAGG_EO_WAVE", "0"),
                       **timed(e, first, last, cand, reps[0], 0 if args.device_only or args.check_only else reps[1],
                               not args.device_only))
        print("ERROR_ONSET_AB " + json.dumps(leg), flush=True)
        legs.append(leg)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/error_onset_ab.py", "unit": "microseconds: the median of five interleaved rounds' "
                       "medians, the fastest and the slowest round (host clock around calls that end in a wait)",
                       "engines": legs}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
