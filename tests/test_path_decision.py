"""The engine's path decision (csrc/sa_path.h: decide_path), without a GPU.

A stand-alone program (its own main, host compiler, no HIP header) reads
configs and prints the path decide_path gives each.  The expected table below
is written from the rules, not from the code:

  cap = next power of two >= 1.25 x key_capacity (>= 16); SA_OPT_DENSE_IDS
        raises it to 2^19
  X   = kLdsExtraBytes = 2048*8 + 32 + 65*32 + 1024*4 + 2048 + 64 = 24,704
  Small        cap*16 + cap*ceil(nbk/2)*4 + X <= 144 KiB, explicit buckets
  ExpoSmall    exponential, cap*41 + X <= 144 KiB, no SA_OPT_EXPO_HBM
  ExpoHbm      any other exponential config
  Dense        SA_OPT_DENSE_IDS
  Binned       nbk <= 17, no ATOMIC_TABLE, 2^19 <= cap <= 2^22, n_windows <=
               1024, a bin table (no power-of-two bin of nanoseconds holds
               more than two thresholds), no SA_OPT_PARTITIONED
  Partitioned  nbk <= 17, no ATOMIC_TABLE, otherwise
  Atomic       the rest

Default bounds: nbk = 17, so Small needs cap*52 + 24,704 <= 147,456: cap <=
2,360, i.e. cap = 2,048 at most, i.e. key_capacity + ceil(key_capacity/4) <=
2,048: 1,638 is the largest (1,638 + 410), 1,639 gives 4,096 slots.

The program also prints the remaining geometry decisions of sa_path.h: the
small-table kernel (small_kernel), the small exponential table's kernel
(expo_kernel), whether the HBM kernels' 16-bound instance applies (bounds16),
the HLL filter's sub-blocks (hll_filter_geometry), the small tables' ERROR
table rule (error_table) and, for an LDS table, where the kernels' LDS layout
(small_lds_layout) ends, which must be the launch's lds_bytes (the list
summed here against the list summed by decide_path: it shows that decide_path
passes the kernel's counter words and EXPO flag, no more).
tests/geometry_util.py states those rules and works every row of its matrix
out by hand; the rows are checked here on the CPU and run on the GPU by
tests/test_gpu_geometry.py.  The rows of the moving-ring matrix (RING_ROWS,
run by tests/test_gpu_ring.py) and the rows for the ends of hll_p
(hll_util.HLL_ROWS, run by tests/test_gpu_hll_ids.py) go through the same
program and the same assertions.

The same program also runs built with -fsanitize=address,undefined (plain
host code; nothing is preloaded).
"""
import os
import shutil
import subprocess

import pytest

from geometry_util import RING_ROWS, ROWS
from hll_util import HLL_ROWS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opentelemetry-demo_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

PARTITIONED, ATOMIC, EXPO_HBM, DENSE = 1 << 1, 1 << 2, 1 << 3, 1 << 9  # SA_OPT_* (include/spanagg.h)
DEFAULT = [2, 4, 6, 8, 10, 50, 100, 200, 400, 800, 1000, 1400, 2000, 5000, 10000, 15000]
TWENTY = DEFAULT + [20000, 30000, 40000, 50000]  # nbk = 21 > kPartMaxBk
CROWDED = [1.1, 1.2, 1.3]  # ms: 1.1e6, 1.2e6, 1.3e6 ns all in [2^20, 2^21): no bin table

# (key_capacity, exp_max_size, options, n_windows, bounds) -> (path, log2 of the table slots)
CASES = [
    ((1000, 0, 0, 8, DEFAULT), ("Small", 11)),
    ((1000, 160, 0, 8, DEFAULT), ("ExpoSmall", 11)),
    ((1000, 160, EXPO_HBM, 8, DEFAULT), ("ExpoHbm", 11)),
    ((1638, 0, 0, 8, DEFAULT), ("Small", 11)),        # the largest default-bounds table in LDS
    ((1639, 0, 0, 8, DEFAULT), ("Partitioned", 12)),  # one more key: 4,096 slots
    ((1638, 160, 0, 8, DEFAULT), ("ExpoSmall", 11)),  # 2,048*41 + X = 108,672
    ((1639, 160, 0, 8, DEFAULT), ("ExpoHbm", 12)),    # 4,096*41 + X = 192,640
    ((1000, 0, 0, 8, CROWDED), ("Small", 11)),        # Small does not need the bin table
    ((200_000, 0, 0, 8, DEFAULT), ("Partitioned", 18)),
    ((300_000, 0, 0, 8, DEFAULT), ("Binned", 19)),
    ((300_000, 0, PARTITIONED, 8, DEFAULT), ("Partitioned", 19)),
    ((300_000, 0, ATOMIC, 8, DEFAULT), ("Atomic", 19)),
    ((300_000, 0, 0, 8, CROWDED), ("Partitioned", 19)),  # no bin table, hence not Binned
    ((3_000_000, 0, 0, 8, DEFAULT), ("Binned", 22)),
    ((4_000_000, 0, 0, 8, DEFAULT), ("Partitioned", 23)),
    ((1_200_000, 0, 0, 1024, DEFAULT), ("Binned", 21)),
    ((1_200_000, 0, 0, 2048, DEFAULT), ("Partitioned", 21)),
    ((1_200_000, 0, 0, 8, TWENTY), ("Atomic", 21)),
    ((1_200_000, 0, 0, 8, TWENTY[:17]), ("Atomic", 21)),       # nbk = 18: the first past kPartMaxBk
    ((1000, 0, DENSE, 8, DEFAULT), ("Dense", 19)),
    ((3_000_000, 0, DENSE, 8, DEFAULT), ("Dense", 22)),
]
LDS = {0: 2048 * 52 + 24704, 1: 2048 * 41 + 24704}  # dynamic LDS of cases 0 (Small) and 1 (ExpoSmall)

PROGRAM = r"""
#include <cstdio>
#include <vector>
#include "sa_path.h"

int main() {
  static const char *names[] = {"Small", "ExpoSmall", "ExpoHbm", "Binned", "Dense", "Partitioned", "Atomic"};
  static const char *small[] = {"small_default", "small_512", "small_1024", "small_linear"};
  static const char *expo[] = {"expo_specialised", "expo_generic"};
  unsigned long long kcap, window_ns;
  unsigned exp_max, options, n_windows, unit, hll_p, n_services, nb;
  while (std::scanf("%llu %u %u %u %u %u %u %llu %u", &kcap, &exp_max, &options, &n_windows, &unit, &hll_p,
                    &n_services, &window_ns, &nb) == 9) {
    std::vector<double> bounds(nb);
    for (double &b : bounds)
      if (std::scanf("%lf", &b) != 1) return 2;
    sa_config c{};
    c.bounds = bounds.data();
    c.n_bounds = nb;
    c.unit = unit;
    c.hll_p = hll_p;
    c.n_windows = n_windows;
    c.n_services = n_services;
    c.window_ns = window_ns;
    c.key_capacity = kcap;
    c.exp_max_size = exp_max;
    c.options = options;
    sa::Hist h;
    if (!sa::build_hist(c.bounds, c.n_bounds, c.unit, h)) return 3;
    const uint64_t cap = sa::config_table_slots(c);
    const uint32_t log2cap = sa::log2u(cap);
    const sa::PathChoice pc = sa::decide_path(c, h, cap);
    const char *kernel = pc.path == sa::Path::Small
                             ? small[(int)sa::small_kernel(h.has_bins, pc.lds_bytes, log2cap, h.nbk, c.hll_p)]
                         : pc.path == sa::Path::ExpoSmall ? expo[(int)sa::expo_kernel(log2cap, c.hll_p)]
                         : sa::bounds16(h.nneg, h.npos)   ? "bounds16"
                                                          : "bounds_generic";
    const sa::LbGeom lb = sa::hll_filter_geometry(c);
    // the small-table kernel's workgroup and spans per lane (0 0: not a Small engine)
    unsigned block = 0, spl = 0, v2 = 0;
    if (pc.path == sa::Path::Small) {
      const sa::SmallKernel k = sa::small_kernel(h.has_bins, pc.lds_bytes, log2cap, h.nbk, c.hll_p);
      block = sa::small_block(k);
      spl = sa::small_spans_per_lane(k);
      v2 = sa::small_is_v2(k);
    }
    // where the kernel's LDS layout ends, walked region by region (0: no LDS table)
    size_t lds_end = 0;
    if (sa::lds_table(pc.path)) {
      const bool x = pc.path == sa::Path::ExpoSmall;
      const sa::SmallLdsLayout layout = sa::small_lds_layout(cap, x ? sa::kExpoWords : (h.nbk + 1) / 2, x);
      for (const sa::LdsRegion &r : layout.r) lds_end += r.n * r.elem;
    }
    std::printf("%s %u %zu %s %u %u %d %u %u %u %u %zu\n", names[(int)pc.path], log2cap, pc.lds_bytes, kernel, lb.shift,
                lb.n, (int)(sa::lds_table(pc.path) && sa::error_table(c.n_windows, cap)), h.nneg, block, spl, v2, lds_end);
  }
  return 0;
}
"""


def _line(key_capacity=1000, exp_max_size=0, options=0, n_windows=8, unit="ms", hll_p=14, n_services=64,
          window_ns=10_000_000_000, bounds=DEFAULT, **sketch):
    """One config as the program reads it (cms_d and cms_w decide nothing here)."""
    assert set(sketch) <= {"cms_d", "cms_w"}, sketch
    return (f"{key_capacity} {exp_max_size} {options} {n_windows} {int(unit == 's')} {hll_p} {n_services} {window_ns} "
            f"{len(bounds)} {' '.join(repr(float(v)) for v in bounds)}\n")


SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


@pytest.mark.parametrize("flags", [[], SANITIZE], ids=["plain", "sanitized"])
def test_path_table(tmp_path, flags):
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    src, exe = tmp_path / "path_decision.cpp", tmp_path / "path_decision"
    if flags:  # the sanitizer runtimes linked statically (clang's default; GCC's spelling otherwise)
        gnu = "clang" not in subprocess.run([cxx, "--version"], capture_output=True, text=True).stdout
        flags = flags + (["-static-libasan", "-static-libubsan"] if gnu else ["-static-libsan"])
    src.write_text(PROGRAM)
    with open(os.path.join(CSRC, "sa_path.h")) as f:
        includes = [ln for ln in f if ln.startswith("#include")]
    assert includes and not [ln for ln in includes if "hip" in ln.lower()], includes
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, "-I", INCLUDE,
                    str(src), "-o", str(exe)], check=True)
    lines = "".join(_line(key_capacity=k, exp_max_size=x, options=o, n_windows=w, bounds=b) for (k, x, o, w, b), _ in CASES)
    lines += "".join(_line(**r["cfg"]) for r in ROWS.values())
    out = subprocess.run([str(exe)], input=lines, capture_output=True, text=True, check=True).stdout.split("\n")
    got = [tuple(ln.split()) for ln in out if ln]
    assert len(got) == len(CASES) + len(ROWS)
    for i, ((cfg, (path, log2cap)), g) in enumerate(zip(CASES, got)):
        assert (g[0], int(g[1])) == (path, log2cap), (cfg[:4], g)
        if i in LDS:
            assert int(g[2]) == LDS[i], (cfg[:4], g)
        _assert_layout_end(g, cfg[:4])
    # the default table is the default geometry: the specialised kernels, the 16-bound instances
    assert [g[3] for g in got[:3]] == ["small_default", "expo_specialised", "bounds16"]
    assert got[7][3] == "small_linear"  # CROWDED on a small table
    assert got[8][3] == "bounds16" and got[17][3] == "bounds_generic"
    _assert_rows(ROWS, got[len(CASES):])
    ring = subprocess.run([str(exe)], input="".join(_line(**r["cfg"]) for r in RING_ROWS.values()),
                          capture_output=True, text=True, check=True).stdout.split("\n")
    ring = [tuple(ln.split()) for ln in ring if ln]
    assert len(ring) == len(RING_ROWS)
    _assert_rows(RING_ROWS, ring)
    ends = subprocess.run([str(exe)], input="".join(_line(**r["cfg"]) for r in HLL_ROWS.values()),
                          capture_output=True, text=True, check=True).stdout.split("\n")
    ends = [tuple(ln.split()) for ln in ends if ln]
    assert len(ends) == len(HLL_ROWS) == 6
    _assert_rows(HLL_ROWS, ends)


def _assert_layout_end(g, what):
    """An LDS table's launch size is where the kernels' layout ends (sa_path.h small_lds_layout)."""
    if g[0] in ("Small", "ExpoSmall"):
        assert int(g[11]) == int(g[2]) > 0, (what, g)
    else:
        assert int(g[11]) == 0, (what, g)


def _assert_rows(rows, got):
    for (name, r), g in zip(rows.items(), got):
        _assert_layout_end(g, name)
        assert (g[0], int(g[1]), g[3]) == (r["path"], r["log2cap"], r["kernel"]), (name, g)
        assert (int(g[4]), int(g[5])) == r["lb"], (name, g)
        assert bool(int(g[6])) == r["error_table"], (name, g)
        if r["lds"]:
            assert int(g[2]) == r["lds"], (name, g)
        assert int(g[7]) == sum(b < 0 for b in r["cfg"].get("bounds", DEFAULT)), (name, g)
        # small tables (geometry_util.assert_geometry's rule on the GPU): 512-thread workgroups for
        # small_512, 1,024 otherwise; 4 spans per lane for the linear-threshold kernel, 2 for the v2 kernels
        if r["path"] == "Small":
            linear = r["kernel"] == "small_linear"
            assert int(g[8]) == (512 if r["kernel"] == "small_512" else 1024), (name, g)
            assert (int(g[9]), int(g[10])) == ((4, 0) if linear else (2, 1)), (name, g)
        else:
            assert (int(g[8]), int(g[9]), int(g[10])) == (0, 0, 0), (name, g)
