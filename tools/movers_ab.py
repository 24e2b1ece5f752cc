#!/usr/bin/env python3
"""Times Engine.window_movers (k = 10) against the two Engine.window_top calls
over the same two ranges -- the closest thing the engine offered before -- in
one process, alternating, host clock around calls that end in their own device
wait.  DESIGN.md section 4, "Movers between two ranges".

  default      synth.generate_c2 on the default engine, 16 windows: windows
               1..3 against windows 4..5
  ring_binned  tests' ring_binned row (a 2^19-slot binned table, 57,646 series,
               4 windows): the ring's halves
  c4           synth.generate_highcard (1,000,000 series, key_capacity
               1,200,000, 16 windows): the ring's halves

--label names the library measured: SPANAGG_LIB selects another build, e.g.
one compiled with -DSA_MOVERS_CELLS_LDS=0 (no LDS staging), and the two runs'
files are compared by hand.  One JSON line per engine, and --out.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "opentelemetry-demo_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]


def timed(e, base, cur, warm, reps):
    mv, tp = [], []
    for i in range(warm + reps):
        t0 = time.perf_counter()
        r = e.window_movers(base, cur, 10)
        t1 = time.perf_counter()
        a = e.window_top(*base, 10)
        b = e.window_top(*cur, 10)
        t2 = time.perf_counter()
        if i >= warm:
            mv.append(t1 - t0), tp.append(t2 - t1)
    q = lambda v: [round(1e6 * x, 1) for x in (statistics.median(v), min(v), statistics.quantiles(v, n=10)[8])]
    return dict(movers_us=q(mv), top_pair_us=q(tp), n_resident=r.n_resident, n_matched=r.n_matched,
                top_matched=[a.n_matched, b.n_matched])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="product")
    ap.add_argument("--engines", default="default,ring_binned,c4")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from spanagg import Config, Engine
    from spanagg.synth import generate_c2, generate_highcard
    legs = []
    for name in args.engines.split(","):
        if name == "default":
            wl = generate_c2(400_003, seed=21)
            cfg, w0, batches = Config(n_services=wl.n_services, n_windows=16), wl.first_window, [wl.batch]
            base, cur = (w0 + 1, w0 + 3), (w0 + 4, w0 + 5)
        elif name == "ring_binned":
            import range_util
            c = range_util.case("full:ring_binned")
            cfg, w0, batches = c.cfg, c.base, [b for _, b in c.steps]
            base, cur = (w0, w0 + 1), (w0 + 2, w0 + 3)
        elif name == "c4":
            hc, _, w0 = generate_highcard(4_000_000, seed=7)
            cfg, batches = Config(n_services=1, n_windows=16, key_capacity=1_200_000), [hc]
            base, cur = (w0, w0 + 7), (w0 + 8, w0 + 15)
        else:
            ap.error(f"unknown engine {name}")
        with Engine(cfg) as e:
            e.window_advance(w0)
            for b in batches:
                e.ingest(b)
            leg = dict(engine=name, lib=args.label, cells=[cfg.cms_d, cfg.cms_w], slots=e.stats()["table_capacity"],
                       base=base, cur=cur, **timed(e, base, cur, args.warmup, args.calls))
        print("MOVERS_AB " + json.dumps(leg), flush=True)
        legs.append(leg)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"tool": "tools/movers_ab.py", "unit": "microseconds: median, fastest, 90th percentile (host clock "
                       "around calls that end in a wait)", "engines": legs}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
