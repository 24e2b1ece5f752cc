// sa_path.h -- which ingest path an engine runs, decided once from its config.
// Plain host C++ (no HIP header): sa_internal.h includes it for the constants
// the kernels share, sa_create takes its decision, and a stand-alone program
// can print it (tests/test_path_decision.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "spanagg.h"

#pragma GCC visibility push(hidden)  // internal to the library
namespace sa {

constexpr int kMaxBounds = 62;          // SA_MAX_BOUNDS

// Bucket lookup table: bin k = floor(log2 d) (k = 64 for d = 0).  For d in
// bin k, bucket = base + [d > ta] + [d > tb] (ta/tb = UINT64_MAX when absent);
// valid when no bin holds more than two thresholds.
struct BinEntry {
  unsigned long long ta, tb;
  uint32_t base, pad[3];
};
constexpr int kBins = 65;

// HLL bound sub-blocks: 2^kLbMinShift registers or more, at most kLbMaxSub of
// them per engine (the kernels keep the bounds in LDS)
constexpr uint32_t kLbMinShift = 10;
constexpr uint32_t kLbMaxSub = 2048;

#ifndef SA_PART_BIN_BITS
#define SA_PART_BIN_BITS 11
#endif
constexpr uint32_t kPartBinBits = SA_PART_BIN_BITS;
constexpr uint32_t kPartMaxBk = 17;       // LDS counter row: nbk <= 17 (default buckets)

constexpr uint32_t kHllQueue = 2048;  // deferred HLL raises per workgroup (8 B each)
constexpr uint32_t kErrTab = 1024;    // LDS (window, slot) -> ERROR count table per workgroup (4 B each)
// The small-table kernels' dynamic LDS: its regions in order, for a table of
// `cap` slots with `nw` u32 counter words per slot (EXPO: nw = 6, so sums +
// counters are the 32-B header partials of a slot).  The one list behind
// decide_path's sizes and kLdsExtraBytes; the kernels' carve (small_lds_carve,
// spanagg_kernels.hip) steps over the same regions by their element counts,
// with pointer types whose sizes it asserts to be the `elem` given here.
// ingest_lds_kernel uses the head, up to the control block's first word.
struct LdsRegion {
  size_t n, elem;  // n elements of elem bytes
};
enum { kLdsKeys, kLdsSums, kLdsCnt, kLdsHq, kLdsCtl, kLdsBins, kLdsErr, kLdsLb, kLdsScale, kLdsReserved, kLdsRegions };
struct SmallLdsLayout {
  LdsRegion r[kLdsRegions];
  constexpr size_t end() const {
    size_t e = 0;
    for (const LdsRegion &x : r) e += x.n * x.elem;
    return e;
  }
};
constexpr SmallLdsLayout small_lds_layout(size_t cap, size_t nw, bool expo) {
  return {{{cap, 8},                      // key mirror
           {cap, 8},                      // ns sums
           {cap * nw, 4},                 // counters
           {kHllQueue, 8},                // HLL queue
           {8, 4},                        // control block: hq_n[4] + lstat[4]
           {kBins, sizeof(BinEntry)},     // bin table
           {kErrTab, 4},                  // ERROR table
           {kLbMaxSub, 1},                // HLL bounds
           {expo ? cap : 0, 1},           // EXPO: the index records' per-slot scales
           // no kernel uses these, but the path decision's thresholds and
           // every recorded geometry count them
           {64, 1}}};
}
constexpr size_t kExpoWords = 6;  // the EXPO kernel's nw
// the LDS beyond the table (what the layout of an empty table holds)
constexpr size_t kLdsExtraBytes = small_lds_layout(0, 0, false).end();
constexpr size_t kLdsBudget = 144 * 1024;  // small-table path LDS ceiling per workgroup

inline uint32_t log2u(uint64_t x) { return 63u - (uint32_t)__builtin_clzll(x); }
inline uint64_t next_pow2(uint64_t x) {
  uint64_t p = 1;
  while (p < x) p <<= 1;
  return p;
}

// Table slots of an engine: the next power of two >= 1.25 x key_capacity;
// dense-index engines raise it to the binned path's smallest table.
inline uint64_t table_slots(uint64_t key_capacity) {
  return std::max<uint64_t>(16, next_pow2(key_capacity + (key_capacity + 3) / 4));
}
inline uint64_t dense_table_slots(uint64_t key_capacity) {
  return std::max<uint64_t>(1ULL << (kPartBinBits + 8), table_slots(key_capacity));
}
inline uint64_t config_table_slots(const sa_config &c) {
  return (c.options & SA_OPT_DENSE_IDS) ? dense_table_slots(c.key_capacity) : table_slots(c.key_capacity);
}

// thr[i] = max{d in u64 : float64(d)/div <= bounds[n_neg + i]} (sa_bucket_thresholds)
inline int bucket_thresholds(const double *bounds, uint32_t n, uint32_t unit, uint64_t *thr, uint32_t *n_neg) {
  if (n > SA_MAX_BOUNDS || (n && (!bounds || !thr)) || !n_neg || unit > SA_UNIT_S)
    return SA_EINVAL;
  for (uint32_t i = 0; i < n; ++i) {
    if (std::isnan(bounds[i])) return SA_EINVAL;
    if (i && !(bounds[i - 1] <= bounds[i])) return SA_EINVAL;
  }
  const double div = unit == SA_UNIT_S ? 1e9 : 1e6;
  uint32_t neg = 0;
  while (neg < n && bounds[neg] < 0.0) ++neg;
  for (uint32_t i = neg; i < n; ++i) {
    const double b = bounds[i];
    // T = max{d in u64 : float64(d)/div <= b}; f(d) is monotone non-decreasing.
    auto f_le = [&](uint64_t d) { return (double)d / div <= b; };
    uint64_t t;
    if (f_le(UINT64_MAX)) {
      t = UINT64_MAX;
    } else {
      uint64_t lo = 0, hi = UINT64_MAX;  // f_le(lo) holds since b >= 0
      while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (f_le(mid)) lo = mid;
        else hi = mid;
      }
      t = lo;
    }
    thr[i - neg] = t;
  }
  *n_neg = neg;
  return SA_OK;
}

// The explicit-bucket histogram of an engine, built once from its config:
// validate_config, sa_create and the device upload all read this one result.
struct Hist {
  std::vector<double> bounds;
  uint64_t thr[kMaxBounds]{};  // u64 nanosecond thresholds of the non-negative bounds
  uint32_t npos = 0, nneg = 0, nbk = 0;
  BinEntry bins[kBins]{};  // bucket bin table for the LDS kernels
  bool has_bins = false;   // false: some bin holds more than 2 thresholds (linear thresholds)
};

// false: the bounds are not sorted ascending or hold a NaN
inline bool build_hist(const double *bounds, uint32_t n_bounds, uint32_t unit, Hist &h) {
  h.nbk = n_bounds + 1;
  if (bucket_thresholds(bounds, n_bounds, unit, h.thr, &h.nneg) != SA_OK) return false;
  h.bounds.assign(bounds, bounds + n_bounds);
  h.npos = n_bounds - h.nneg;
  h.has_bins = true;
  for (int k = 0; k < kBins; ++k) {
    h.bins[k] = BinEntry{UINT64_MAX, UINT64_MAX, h.nneg, {0, 0, 0}};
    if (k == 64) continue;  // d = 0: no u64 threshold is below 0
    const uint64_t lo = 1ULL << k, hi = k == 63 ? UINT64_MAX : (2ULL << k) - 1;
    uint32_t below = 0, inside = 0;
    for (uint32_t i = 0; i < h.npos; ++i) {
      const uint64_t t = h.thr[i];
      if (t < lo) ++below;                  // every d in the bin exceeds it
      else if (t < hi) {                    // decided per span
        if (inside == 0) h.bins[k].ta = t;
        else if (inside == 1) h.bins[k].tb = t;
        ++inside;
      }
    }
    if (inside > 2) {
      h.has_bins = false;
      break;
    }
    h.bins[k].base = h.nneg + below;
  }
  return true;
}

enum class Path { Small, ExpoSmall, ExpoHbm, Binned, Dense, Partitioned, Atomic };
constexpr bool binned_like(Path p) { return p == Path::Binned || p == Path::Dense; }
constexpr bool expo_like(Path p) { return p == Path::ExpoSmall || p == Path::ExpoHbm; }
constexpr bool lds_table(Path p) { return p == Path::Small || p == Path::ExpoSmall; }

struct PathChoice {
  Path path;
  size_t lds_bytes;  // the ingest kernel's dynamic LDS (Small, ExpoSmall)
};

// The path of a validated config with `cap` table slots (config_table_slots).
inline PathChoice decide_path(const sa_config &c, const Hist &h, uint64_t cap) {
  const bool expo = c.exp_max_size != 0;
  const size_t lds = small_lds_layout(cap, (h.nbk + 1) / 2, false).end();
  if (lds <= kLdsBudget && !expo) return {Path::Small, lds};
  if (expo) {
    const size_t xl = small_lds_layout(cap, kExpoWords, true).end();
    if (xl <= kLdsBudget && !(c.options & SA_OPT_EXPO_HBM)) return {Path::ExpoSmall, xl};
    return {Path::ExpoHbm, lds};
  }
  // dense-index engines (validate_config checked the geometry): the binned
  // path's tables and pipeline with the dense kernels
  if (c.options & SA_OPT_DENSE_IDS) return {Path::Dense, lds};
  // partitioned path unless the LDS counter row is too small for the
  // buckets (SA_OPT_ATOMIC_TABLE: per-span atomics)
  if (h.nbk > kPartMaxBk || (c.options & SA_OPT_ATOMIC_TABLE)) return {Path::Atomic, lds};
  // binned-table path where each bin's sub-table fits an aggregate
  // workgroup's LDS (256..2048 slots per bin: 2^19..2^22 table slots), the
  // window slot fits the record (<= 1024 windows) and buckets come from the
  // bin table (SA_OPT_PARTITIONED: the partitioned path)
  const uint32_t log2cap = log2u(cap);
  const bool binned = log2cap >= kPartBinBits + 8 && log2cap <= kPartBinBits + 11 && c.n_windows <= 1024 &&
                      h.has_bins && !(c.options & SA_OPT_PARTITIONED);
  return {binned ? Path::Binned : Path::Partitioned, lds};
}

// The geometry the specialised small-table kernels are compiled for: 2,048
// slots, 17 or 18 buckets (9 u16-pair counter words per slot), HLL p = 14.
constexpr bool default_geometry(uint32_t log2cap, uint32_t nbk, uint32_t hll_p) {
  return log2cap == 11 && (nbk + 1) / 2 == 9 && hll_p == 14;
}

// Which small-table kernel a Small engine runs (spanagg_kernels.hip product_small_fn):
// the linear-threshold kernel for bounds no bin table holds; otherwise the v2
// kernel -- specialised for the default geometry, generic with 512-thread
// workgroups where the LDS state fits a CU's 160 KiB twice (two workgroups per
// CU: one's prologue and write-back overlap the other's loop, DESIGN section
// 4), generic with 1,024 threads for the rest.
enum class SmallKernel { Default, Generic512, Generic1024, Linear };
inline SmallKernel small_kernel(bool has_bins, size_t lds_bytes, uint32_t log2cap, uint32_t nbk, uint32_t hll_p) {
  if (!has_bins) return SmallKernel::Linear;
  if (default_geometry(log2cap, nbk, hll_p)) return SmallKernel::Default;
  return 2 * lds_bytes <= (size_t)160 * 1024 ? SmallKernel::Generic512 : SmallKernel::Generic1024;
}
// Its workgroup, the spans a lane takes per tile (block x spans = the least a
// workgroup is given), and whether it is the v2 kernel (u16 LDS counters for a
// whole launch, per-workgroup ERROR slabs) or the linear-threshold one.
constexpr uint32_t small_block(SmallKernel k) { return k == SmallKernel::Generic512 ? 512u : 1024u; }
constexpr uint32_t small_spans_per_lane(SmallKernel k) { return k == SmallKernel::Linear ? 4u : 2u; }
constexpr bool small_is_v2(SmallKernel k) { return k != SmallKernel::Linear; }

// The small exponential table's kernel: specialised for 2,048 slots and HLL
// p = 14 (the buckets live in HBM, so their number does not matter).
enum class ExpoKernel { Specialised, Generic };
constexpr ExpoKernel expo_kernel(uint32_t log2cap, uint32_t hll_p) {
  return log2cap == 11 && hll_p == 14 ? ExpoKernel::Specialised : ExpoKernel::Generic;
}

// The HBM-table kernels (per-span atomics, the partitioned scatter) have an
// instance unrolled for 16 non-negative bounds and a generic one.
constexpr bool bounds16(uint32_t nneg, uint32_t npos) { return nneg == 0 && npos == 16; }

// HLL lower-bound filter: one bound per sub-block of 2^shift registers, the
// sub-blocks as small as kLbMinShift allows within kLbMaxSub of them and never
// larger than one service's 2^hll_p registers.  n = 0: no filter (hll_p below
// kLbMinShift, too many registers, or SA_OPT_NO_HLL_FILTER).
struct LbGeom {
  uint32_t shift, n;
};
inline LbGeom hll_filter_geometry(const sa_config &c) {
  const uint64_t regs = (uint64_t)c.n_windows * c.n_services << c.hll_p;
  uint32_t sh = kLbMinShift;
  while (sh < c.hll_p && (regs >> sh) > kLbMaxSub) ++sh;
  if ((regs >> sh) <= kLbMaxSub && sh <= c.hll_p && !(c.options & SA_OPT_NO_HLL_FILTER))
    return {sh, (uint32_t)(regs >> sh)};
  return {0, 0};
}

// The v2 and exponential small-table kernels' per-workgroup LDS ERROR table
// (errslab) keys a (window, slot) pair in 16 bits; engines with more pairs
// count ERROR spans per span instead.
constexpr bool error_table(uint32_t n_windows, uint64_t cap) { return (uint64_t)n_windows * cap < 65535; }

}  // namespace sa
#pragma GCC visibility pop
