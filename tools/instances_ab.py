#!/usr/bin/env python3
"""One timing round of the small-table kernel instances bench.py does not run.

The C2 batch (10 M spans, ~1,400 series, every key resident: the hot loop, no
cold lookups) through one engine per instance, each chosen by its config and
checked against sa_debug_geometry:

  small_512      3 bounds (2 counter words per slot): 2,048 slots fit LDS twice
  small_1024     default bounds, HLL p 12 (not the default geometry)
  expo_generic   exponential histograms, HLL p 12
  small_linear   bounds no bin table holds (three thresholds in one octave)
  lab_diag       INSTANCES_LAB=1 with libspanagg_ab.so: the ablation instance
                 with no ablation bit set (flag 65536 is unused)

Prints one JSON line {instance: us per launch} (10 launches after a warm one,
HIP events, best of two interleaved passes).  To compare two builds, alternate
them through SPANAGG_LIB, one process per build and round:

  for r in 1 2 3 4 5; do for lib in OLD.so NEW.so; do
    SPANAGG_LIB=$lib python tools/instances_ab.py; done; done
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opentelemetry-demo_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from spanagg import Config, Engine  # noqa: E402
from spanagg.synth import generate_c2  # noqa: E402

CONFIGS = {
    "small_512": ("small_512", dict(bounds=[10.0, 100.0, 1000.0])),
    "small_1024": ("small_1024", dict(hll_p=12)),
    "expo_generic": ("expo_generic", dict(hll_p=12, exp_max_size=160)),
    "small_linear": ("small_linear", dict(bounds=[1.1, 1.2, 1.3])),
}
if os.environ.get("INSTANCES_LAB"):
    CONFIGS = {"lab_diag": ("lab", dict(flags=65536))}


def main():
    n = int(os.environ.get("INSTANCES_SPANS", 10_000_000))
    wl = generate_c2(n, seed=42)
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(dev)
            for c in wl.batch.columns()]
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    engines, geometry = {}, {}
    for name, (kernel, kw) in CONFIGS.items():
        e = Engine(Config(n_services=wl.n_services, n_windows=16, key_capacity=1000, **kw))  # 2,048 slots
        e.window_advance(wl.first_window)
        g = e.debug_geometry()
        assert g["kernel"] == kernel, (name, g)
        geometry[name] = [g["path"], g["kernel"], g["block"], g["lds_bytes"]]
        engines[name] = e
    reps, us = 10, {}
    for rnd in range(3):  # the first pass warms up
        for name, e in engines.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e.ingest_device(*cols, n=n, stream=stream.cuda_stream)
            a.record(stream)
            for _ in range(reps):
                e.ingest_device(*cols, n=n, stream=stream.cuda_stream)
            b.record(stream)
            b.synchronize()
            if rnd:
                us.setdefault(name, []).append(a.elapsed_time(b) / reps * 1e3)
    dropped = {name: e.stats()["dropped_table_full"] for name, e in engines.items()}  # (0: no span took the full-table path)
    print(json.dumps({"lib": os.path.basename(os.environ.get("SPANAGG_LIB", "libspanagg.so")), "spans": n,
                      "geometry": geometry, "dropped": dropped, "us": {k: min(v) for k, v in us.items()}}))
    for e in engines.values():
        e.close()


if __name__ == "__main__":
    main()
