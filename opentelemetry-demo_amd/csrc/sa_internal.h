// sa_internal.h -- shared definitions between the HIP kernels and the C-ABI
// engine of libspanagg (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sa_path.h"  // constants the path decision shares: BinEntry, kBins, kLdsExtraBytes, ...
#include "sa_probe.h"  // the key tables' probe sequences: probe_seq, seq_slot, bt_seq, bt_pos, part_bin, ...

namespace sa {

constexpr uint32_t kNotFound = 0xFFFFFFFFu;
constexpr uint64_t kPhi = 0x9E3779B97F4A7C15ULL;  // Fibonacci hashing multiplier

// stats slots (device array of u64)
enum : int {
  kStatZeroKey = 0,
  kStatInvalidService = 1,
  kStatWindowOOR = 2,
  kStatDropped = 3,
  kNumStats = 4
};
// HLL updates skipped by the lower-bound filter (sa_stats.hll_filtered): one
// u64 slot per workgroup index (mod kFiltSlots), summed when stats are read
constexpr uint32_t kFiltSlots = 1024;

struct XHdr;
struct ExpoHdr;
// Everything the ingest kernels need, passed by value (kernel-argument segment,
// read through the scalar cache).
struct IngestParams {
  // SoA v1 batch (device pointers, 16-B aligned)
  const uint64_t *key, *start, *end, *w0, *w1;
  const uint32_t *meta;
  uint64_t n;
  uint64_t wg_chunk;  // spans per workgroup (multiple of 4; host-computed, = kernel wg_range)
  // key table (open addressing, linear probing, EMPTY = 0)
  unsigned long long *gkeys;
  uint32_t log2cap;
  uint32_t max_probe;
  // small-table path: per-workgroup slabs [G][cap][nbk] u32 and [G][cap] u64
  uint32_t *slab_cnt;
  unsigned long long *slab_sum;
  // HBM-table path: counters [cap][nbk+1] u64 (last = sum_ns); binned path:
  // 32-B rows (kRowBytes) plus the u64 spill array base64 [cap][nbk + 1]
  unsigned long long *gcounts;
  unsigned long long *base64;
  // histogram: bucket(d) = nneg + #{i < npos : d > thr[i]}
  uint64_t thr[kMaxBounds];
  uint32_t npos, nneg, nbk;
  uint32_t epoch_tiles;  // small path: LDS u16 counters flushed every epoch_tiles tiles
  // sketches
  uint8_t *hll;                 // [W][S][2^p]
  unsigned long long *cms;      // [W][d][w]
  unsigned long long *errcnt;   // [W][cap] exact ERROR-span counts per (window, key slot)
  // v2 kernels: per-workgroup ERROR counts [G][W << log2cap] u32, gathered in an
  // LDS table during the launch and added here at its end (nullptr: errcnt atomics)
  uint32_t *errslab;
  uint64_t window_ns, win_magic, win_base;
  uint64_t base_ns, ring_ns;  // win_base * window_ns, n_windows * window_ns (< 2^63)
  float inv_window;           // 1 / window_ns
  // 0.5 - n_windows * 2^-20: a quotient estimate inside the ring whose
  // fraction lies within this of 1/2 has the exact floor (window_slot_lean)
  float win_ok;
  uint32_t base_slot;         // win_base & win_mask
  const BinEntry *bintab;     // [kBins] or nullptr (linear thresholds)
  uint32_t win_mask, n_windows;
  uint32_t p, n_services, cms_d, cms_shift, cms_w;
  uint32_t diag;  // SA_DIAG_* ablation bits (0 in production)
  const uint64_t *seeds;  // [8] count-min row seeds (device memory)
  unsigned long long *stats;
  unsigned long long *dbg;  // diagnostic timestamps [G][8] (nullptr in production)
  // partitioned HBM-table path: span records binned by key ([kPartBins][part_cap]
  // of {key, ns << 7 | bucket}) and the per-bin fill counters
  ulonglong2 *part_rec;
  uint32_t *part_fill;
  uint32_t part_cap;
  // binned-table path (spanagg_binned.hip): key table split into kPartBins
  // bin-local sub-tables of 2^log2sb slots, keys stored as m = key * kmul,
  // u32 count rows; records in per-(bin, scatter workgroup) regions of
  // bt_region records, region fills in bt_cnt [bin][scatter workgroup]
  uint32_t log2sb;
  uint32_t bt_region;
  uint64_t kmul, kinv;
  ulonglong2 *bt_rec;
  uint32_t *bt_cnt;
  uint32_t bt_grid;  // scatter workgroups (regions per bin)
  // the aggregate's second record set (nullptr: one): the next launch's
  // scatter output, aggregated with this one (sa_engine::bt_pend)
  ulonglong2 *bt_rec2;
  uint32_t *bt_cnt2;
  uint32_t bt_grid2, bt_region2;
  // HLL lower bounds: hll_lb[j] <= every register of sub-block j (registers
  // [j << lb_shift, (j + 1) << lb_shift)), so a span whose rho is at most its
  // sub-block's bound cannot raise a register and skips the register read.
  // lb_n sub-blocks (0: no filter); lb_seq rotates which sub-blocks a launch
  // refreshes (registers only grow between window clears, which zero the
  // window's bounds, so a bound read at any time stays a lower bound).
  uint8_t *hll_lb;
  uint32_t lb_shift, lb_n, lb_seq;
  unsigned long long *hll_filt;  // [kFiltSlots] (sa_stats.hll_filtered)
  // exponential-histogram engines on the small-table kernel (EXPO): the key
  // slot of every span (for the bucket-counting pass) and the per-workgroup
  // header slabs [G][cap] (XHdr) the rescale pass reduces
  uint32_t *slot_of;  // EXPO mode: [n] key slot of each span (kNotFound without one)
  // EXPO mode with slab counting: [n] span records instead (span_rec_of), so
  // the counting pass reads 8 B per span instead of the slot and both times
  unsigned long long *span_rec;
  unsigned long long *span_long;  // [n]: the duration of each span whose record holds kSpanRecDurMask
  // EXPO mode, index records (xidx != 0): slot_of holds ixrec words -- each
  // span's bucket index at the scale its series had when the kernel started
  // (xscale[], read in the prologue) -- and span_long the durations the
  // fast index path declined
  const int8_t *xscale;  // [cap] each slot's scale (expo_reduce_rescale_kernel keeps it)
  int32_t l2d_q24;  // log2(div) * 2^24 rounded (expo_index_fast)
  uint32_t xidx;
  XHdr *xslab;
};
// One workgroup's exponential-histogram header partial for one key slot
// (EXPO kernel -> expo_reduce_rescale_kernel): counts, exact ns sum, the
// largest ~d over positive durations (so the minimum starts from a zeroed
// slab) and the largest positive duration.
struct XHdr {
  uint32_t cnt, zero;
  unsigned long long sum, minx, max;
};

// Exponential-histogram mode (spanagg_expo.hip): per key slot a header and
// max_size u32 buckets kept circularly (index mod max_size), two buffers so a
// downscale can merge from one into the other.
struct ExpoHdr {
  unsigned long long count, zero, sum_ns, min_ns, max_ns, minpos_ns, maxpos_ns;
  int32_t scale, lo, hi;  // the kept buckets' scale and positive index range (lo = INT32_MAX: none)
  uint32_t cur;           // which bucket buffer holds them
};
struct ExpoRow {  // one flushed series
  unsigned long long count, zero, sum_ns, min_ns, max_ns;
  int32_t scale, offset;
  uint32_t n, pad;
};
struct ExpoParams {
  const uint64_t *key, *start, *end;
  uint64_t n;
  unsigned long long *gkeys;
  uint32_t log2cap, max_probe;
  uint64_t cap;
  ExpoHdr *hdr;
  uint32_t *buckets;  // [2][cap][max_size]
  uint32_t max_size;
  double div;         // 1e6 (ms) or 1e9 (s)
  int32_t log2div_q24;  // log2(div) * 2^24 rounded, for the bucket index's fast path
  uint32_t diag;      // ablation bits (SPANAGG_XC_DIAG, profiling only; results wrong when set):
                      // 1 no HBM bucket atomics, 2 no LDS cache, 4 exact index path only, 8 no index
  uint32_t *slot_of;  // [n] key slot of each span (pass 1 / the small-table ingest kernel -> counting)
  const unsigned long long *span_rec;  // [n] span records (slab counting: the small-table kernel -> counting)
  const unsigned long long *span_long;  // [n] durations of the records holding kSpanRecDurMask
  uint32_t xidx;  // slot_of holds index records (ixrec), the counting pass shifts them to the new scale
  int8_t *xscale;  // [cap] each slot's scale as the reduce pass left it, for the ingest kernel (nullptr: none)
  unsigned long long *dropped;
  XHdr *xslab;        // small-table engines: [xG][cap] per-workgroup header partials (nullptr: pass 1 atomics)
  uint32_t xG;
  // small-table bucket counting (expo_count_slab with its entry selection / expo_fold_slab):
  uint32_t *lcount;         // [cap] this launch's positive durations per slot (reduce -> selection)
  int2 *xmeta;              // [cap] {scale | buffer << 8, lo - (lo mod max_size)} per slot (reduce -> counting)
  uint32_t *slot_of_entry;  // [xc_ne] the entry's slot, ~0u: unused (this launch's selection)
  int32_t *xent;            // [cap] each slot's entry, -1: none (this launch's selection)
  int32_t *xent_next;       // [cap] and the next launch's, by the counting kernel's workgroup 0
  uint32_t *soe_next;       // [xc_ne] the next launch's slot_of_entry
  uint32_t *xcslab;         // [xG][xc_slab_stride] per-workgroup u16 bucket-count pairs ([xc_ne][(max_size + 1) / 2])
  uint32_t xc_ne;           // LDS entries of the counting kernel (0: the cached-probe kernel)
  // the counting kernel's tail (spans of series without an LDS entry): each
  // workgroup's (slot << 12 | bucket) records, sorted by fold bin of
  // xt_bin_slots slots, each bin's run at a fixed place [xG][nbins][kXtRun],
  // and the runs' lengths [xG][nbins + 1];
  // expo_fold_kernel sums them per bin (nullptr: HBM atomics)
  uint32_t *xt_rec, *xt_off;  // (records past kXtCap, or past a full run, take an HBM atomic)
  // SA_OPT_STAMPS: the counting kernel's per-workgroup s_memrealtime stamps,
  // in the ingest kernel's stamp rows (kDbgPerWg per workgroup; slots
  // kXcStamp.. are the counting kernel's); nullptr: none
  unsigned long long *dbg;
};
// A span record of the exponential-histogram slab path: the key slot in the
// top 12 bits (kSpanRecNoSlot: none; slab tables have <= 2,048 slots) and the
// duration in ns below; a duration of 2^52 - 1 ns (52 days) or more is stored
// as kSpanRecDurMask and in full at the span's index of span_long (so the
// counting pass reads no caller memory).
constexpr uint32_t kSpanRecShift = 52;
constexpr uint32_t kSpanRecNoSlot = 0xFFFu;
constexpr unsigned long long kSpanRecDurMask = (1ull << kSpanRecShift) - 1;
__host__ __device__ inline unsigned long long span_rec_of(uint32_t slot, unsigned long long d) {
  return (unsigned long long)(slot < kSpanRecNoSlot ? slot : kSpanRecNoSlot) << kSpanRecShift |
         (d < kSpanRecDurMask ? d : kSpanRecDurMask);
}
// An index record (the exponential slab path's span word, u32): the key slot
// in the top 12 bits (kSpanRecNoSlot: none), the scale the ingest kernel read
// for the slot + 10 (5 bits), the bucket index at that scale (14 bits,
// signed) and a flag bit.  Flag with index field 0: the duration is in
// span_long (the fast path declined, or the index needs more bits); flag with
// index field 1: zero duration.  A series' scale only falls within a flush
// interval, so the counting pass gets the index at the scale the reduce pass
// settled on by an arithmetic shift (go-expohisto: bucket i at scale s - 1
// holds buckets 2i and 2i + 1 at scale s).
constexpr uint32_t kIxSlotShift = 20, kIxScaleShift = 15, kIxScaleBias = 10;
constexpr int32_t kIxMin = -(1 << 13), kIxMax = (1 << 13) - 1;
constexpr uint32_t kIxLong = 1u, kIxZero = 3u;  // flag | index field 0 / 1
__host__ __device__ inline uint32_t ixrec_of(uint32_t slot, int32_t scale, int32_t ix) {
  return slot << kIxSlotShift | (uint32_t)(scale + (int32_t)kIxScaleBias) << kIxScaleShift | ((uint32_t)ix & 0x3FFFu) << 1;
}
// log2(div) in the fast bucket index's 8.24 fixed point (expo_index_fast)
__host__ inline int32_t expo_l2d_q24(double div) { return (int32_t)std::llround(std::log2(div) * 16777216.0); }
constexpr uint32_t kXtCap = 4096;       // tail records per counting workgroup (16 KiB of LDS)
constexpr uint32_t kXtRun = 64;         // a counting workgroup's records of one fold bin (C2: ~23 on average)
// slots per tail fold bin: 16 (a fold workgroup counts [16][max_size] u32 in
// LDS), 8 past max_size 2,048; one fold round at C2's 2,048 slots (128 bins)
constexpr uint32_t kXtBinSlotsMax = 16;
__host__ __device__ inline uint32_t xt_bin_slots(uint32_t max_size) { return max_size <= 2048 ? 16u : 8u; }
__host__ __device__ inline uint32_t xt_bins(uint64_t cap, uint32_t max_size) {
  return (uint32_t)((cap + xt_bin_slots(max_size) - 1) / xt_bin_slots(max_size));
}
// the counting slab's words per workgroup: xc_ne entries of (max_size + 1) / 2
// u16 pairs, padded to 16 B (the fold reads four words a lane)
__host__ __device__ inline uint32_t xc_slab_stride(uint32_t ne, uint32_t max_size) {
  return (ne * ((max_size + 1) / 2) + 3u) & ~3u;
}
__host__ __device__ ExpoHdr expo_hdr_empty();
constexpr uint32_t kExpoMaxSize = 4096;

constexpr uint64_t kHostChunkSpans = 1ull << 20;  // sa_ingest pinned slot (44 MiB)
constexpr uint64_t kHostPageableMin = 1ull << 18;  // chunks from here on: the runtime's pageable staging


// Partitioned HBM-table path (high cardinality): part_scatter_kernel bins
// every span's record by the top 11 bits of its key, part_aggregate_kernel
// aggregates one bin per workgroup in an LDS table and adds it to the HBM
// counters once per key.
// (kPartBinBits, kPartMaxBk: sa_path.h)
constexpr uint32_t kPartBins = 1u << kPartBinBits;
// LDS table slots per bin: ~2x the mean keys per bin at 1 M keys
constexpr uint32_t kPartSlotBits = 21 - kPartBinBits;
constexpr uint32_t kPartSlots = 1u << kPartSlotBits;
// records staged per bin in the scatter's LDS (one chunk = kPartStage x 16 B)
#ifndef SA_PART_STAGE
#define SA_PART_STAGE (SA_PART_BIN_BITS >= 11 ? 2 : 8)  // 2: LDS left for a 512-entry overflow table
#endif
constexpr uint32_t kPartStage = SA_PART_STAGE;
constexpr uint32_t kPartBlock = 1024;     // scatter
constexpr uint32_t kPartMaxGrid = 256;    // scatter workgroups per launch, at most
constexpr uint32_t kPartAggBlock = kPartSlots >= 2048 ? 1024 : 512;  // aggregate workgroup
constexpr uint64_t kPartMaxSpans = 1ULL << 24;  // spans per partitioned launch
// records per bin: 1.25x the mean plus slack (a fuller bin spills to the direct path)
constexpr uint64_t kPartMaxCap = kPartMaxSpans / kPartBins * 5 / 4 + 64;  // a multiple of kPartStage
// a bin holds < 2^16 records, so its LDS bucket counters are u16 pairs
static_assert(kPartMaxCap < 65536, "u16 LDS counters");
constexpr uint32_t kPartWords = (kPartMaxBk + 1) / 2;
// (part_bin: sa_probe.h)
constexpr size_t kPartLdsBytes = (size_t)kPartSlots * (16 + 4 * kPartWords);  // 52 KiB at 1,024 slots
// scatter: cur, lim, stage counts (u32 per bin) + a 4-record stage per bin
// scatter overflow table: spans whose bin run is full are pre-aggregated per
// workgroup (key, ns sum, u32 bucket counts) and leave as one row update each
#ifndef SA_PART_HOT_BITS
#define SA_PART_HOT_BITS 9
#endif
constexpr uint32_t kPartHotBits = SA_PART_HOT_BITS;
constexpr uint32_t kPartHot = 1u << kPartHotBits;
constexpr size_t kPartScatterLds =
    (size_t)kPartBins * (12 + kPartStage * 16) + (size_t)kPartHot * (16 + 4 * kPartMaxBk);  // 130 KiB

// Counter row layout (gcounts, one row per key slot): 64-B segments of 8 u64
// cells -- cell 0 holds that segment's share of the ns sum, cells 1..7 seven
// bucket counts.  A span's count cell and sum cell share a segment, so when
// one wave instruction carries both (two adjacent lanes) the memory side
// handles them as one atomic request (tools/atomic_probe.hip: 2x the rate).
// The row's ns sum is the sum of its segments' cells.
constexpr uint32_t kSegBuckets = 7;
__host__ __device__ inline uint32_t row_stride(uint32_t nbk) {
  return (nbk + kSegBuckets - 1) / kSegBuckets * 8;
}
__host__ __device__ inline uint32_t row_count_cell(uint32_t b) {
  return b / kSegBuckets * 8 + 1 + b % kSegBuckets;
}
__host__ __device__ inline uint32_t row_sum_cell(uint32_t b) { return b / kSegBuckets * 8; }

// ---------------------------------------------------------------------------
// Binned key table (high-cardinality path, spanagg_binned.hip): its layout and
// probe sequence (kBinShift, bt_seq, bt_pos, bt_probe_max, bt_slot) are in
// sa_probe.h.
constexpr uint64_t kBinRest = (1ULL << kBinShift) - 1;     // m's bits below the bin
// Counter rows of the binned path: 32 B per key slot, the u64 ns sum then one
// u8 count per bucket (bytes 8 .. 8 + nbk), so two rows share a 64-B half
// line and the aggregate's row read-modify-write moves 32 B per touched key.
// A count that would pass 255 leaves the row: the aggregate adds the row's
// counts to the u64 spill array base64 [cap][nbk + 1] (atomics) and zeroes
// them; the scatter's direct path and overflow table add to base64 directly
// (its last cell is their ns sum).  A key's totals are row + base64.
constexpr uint32_t kRowBytes = 32;
constexpr uint32_t kRowMaxBk = kRowBytes - 8;
static_assert(kPartMaxBk <= kRowMaxBk, "binned rows hold every bucket count");
// Record duration word: the duration in ns (bits 0-58) and its histogram
// bucket (bits 59-63, from the scatter's bin table), so the aggregate needs no
// bucketing; a span of 2^59 ns or longer (18 years) takes the overflow path.
constexpr uint32_t kRecDurBits = 59;
constexpr uint64_t kRecDurMask = (1ULL << kRecDurBits) - 1;
constexpr uint32_t kBtStage = 4;     // records per bin stage: one 64-B chunk per flush
constexpr uint32_t kBtHq = 256;      // scatter deferred HLL raises
constexpr uint32_t kBtBlock = 1024;  // scatter workgroup
constexpr uint32_t kBtMaxWgSpans = 65520;  // u16 claim / overflow counters per scatter workgroup
// round-synchronous scatter (bt_scatter2_kernel): per bin a 4-record stage,
// a u16 claim count (pairs) and a u16 region fill; per wave a flush list of
// 128 bins; the overflow table; HLL queue; bin table; HLL bounds
constexpr uint32_t kBt2Hot = 240;
constexpr uint32_t kBt2HotErr = 128;  // (window slot, overflow entry) -> ERROR count
constexpr size_t kBt2ScatterLds = (size_t)kPartBins * (kBtStage * 16 + 2 + 2) + (kBtBlock / 64) * 128 * 2 +
                                  (size_t)kBt2Hot * (16 + 4 * kPartWords) + (size_t)kBtHq * 8 + 16 +
                                  (size_t)kBins * sizeof(BinEntry) + kLbMaxSub + kBt2HotErr * 8;
static_assert(kBt2ScatterLds <= 163840, "binned scatter2 LDS");
// Dense-index form of the binned path (spanagg_dense.hip, SA_OPT_DENSE_IDS):
// 8-B records in 8-record stages (one 64-B chunk per flush; the stages take
// the LDS of the binned scatter's 4 x 16 B, so kBt2ScatterLds serves both)
// (SA_DN_STAGE=4: 32-B chunks, for A/B builds -- DESIGN.md has the measurement)
#ifndef SA_DN_STAGE
#define SA_DN_STAGE 8
#endif
constexpr uint32_t kDnStage = SA_DN_STAGE;
static_assert(kDnStage == 4 || kDnStage == 8, "dense stage: 4 or 8 records");
static_assert(kDnStage * 8 <= kBtStage * 16, "dense stages fit the binned scatter's LDS layout");

// Geometry of the counter rows and key table for the flush-time kernels
// (compact, gather, count-min fold): both table layouts, both row layouts.
struct RowGeom {
  uint32_t nbk;
  uint32_t row8;    // 1: 32-B u8-count rows + base64 (binned path), 0: u64 segment rows
  uint32_t binned;  // 1: binned key table
  uint32_t log2cap, log2sb, max_probe;
  uint64_t kmul, kinv;            // key <-> stored id (1, 1 unless binned)
  unsigned long long *base64;     // row8: u64 [cap][nbk + 1] spilled counts and sums
  // dense-index engines (SA_OPT_DENSE_IDS): a slot's key is the hash bound to
  // its index, 0 while unbound; the spans of a non-zero row without a key are
  // counted in *dropped when the row is reset
  uint32_t dense;
  unsigned long long *dropped;
};

// (the key table's layout and probe sequence -- ProbeSeq, probe_seq, seq_slot,
// max_probe_of: sa_probe.h)

// HBM-table kernel (ingest_hbm_kernel): 256 threads, 4 spans per lane per tile
constexpr uint32_t kHbmBlock = 256;
constexpr int kHbmSpansPerLane = 4;
// v2 kernels keep u16 LDS counters for a whole launch: spans per workgroup per launch
constexpr uint32_t kMaxWgSpans = 65532;
constexpr uint32_t kDbgPerWg = 136;  // diagnostic stamps per workgroup: 8 + 16 waves x 8
// the exponential counting kernel's stamps in the same rows (slots the ingest
// kernel leaves free): start, prologue done, loop done, end at 4..7; its slab
// stores issued, its LDS zeroed and its entry selection done (thread 0) in
// the last slots of the wave rows
constexpr uint32_t kXcStamp = 4, kXcStampSlab = kDbgPerWg - 1, kXcStampZeroed = kDbgPerWg - 9,
                   kXcStampSelected = kDbgPerWg - 17, kXcStampTail = kDbgPerWg - 25;
// (kHllQueue, kErrTab, small_lds_layout, kLdsExtraBytes: sa_path.h)

// launchers of the small-table path (spanagg_kernels.hip): the engine's kernel
// k (sa_path.h), block small_block(k); diag (laboratory build only): the
// ablation instance in its place, which has Generic1024's geometry.
hipError_t launch_ingest_small(const IngestParams &P, uint32_t grid, size_t lds_bytes, hipStream_t s, SmallKernel k,
                               bool diag);
hipError_t prepare_ingest_small(size_t lds_bytes);
void ingest_small_node(uint32_t grid, size_t lds_bytes, SmallKernel k, void **args, hipKernelNodeParams *np);
uint32_t ingest_small_blocks_per_cu(SmallKernel k, bool diag, size_t lds_bytes);
// exponential-histogram engines with an LDS-sized key table: the small-table
// kernel in EXPO mode (header partials + per-span slots; spanagg_expo.hip
// reduces and counts)
hipError_t prepare_ingest_expo_small(size_t lds_bytes);
hipError_t launch_ingest_expo_small(const IngestParams &P, uint32_t grid, size_t lds_bytes, hipStream_t s);
uint32_t ingest_expo_blocks_per_cu(uint32_t log2cap, uint32_t p, size_t lds_bytes);
// HBM-table paths (spanagg_part.hip): per-span atomics, round-1 partitioned
hipError_t launch_ingest_hbm(const IngestParams &P, uint32_t grid, hipStream_t s);
hipError_t launch_ingest_part(const IngestParams &P, hipStream_t s);
hipError_t prepare_ingest_part();
// flush-time table kernels (spanagg_table.hip)
hipError_t launch_reduce_errslab(uint32_t *errslab, uint32_t G, uint64_t per_wg, uint64_t ws,
                                 uint32_t log2cap, unsigned long long *errcnt_ws, hipStream_t s);
hipError_t launch_count_keys(const unsigned long long *gkeys, uint64_t cap,
                             unsigned long long *out, hipStream_t s);
hipError_t launch_reduce_slabs(uint32_t *slab_cnt, unsigned long long *slab_sum,
                               unsigned long long *gcounts, uint32_t G, uint64_t cap,
                               uint32_t nbk, hipStream_t s);
hipError_t launch_compact(const unsigned long long *gkeys, unsigned long long *gcounts,
                          uint64_t cap, const RowGeom &g, unsigned long long *out_keys,
                          unsigned long long *out_rows, unsigned long long *out_n,
                          uint64_t out_cap, int reset, hipStream_t s);
hipError_t launch_gather_dense(const unsigned long long *gkeys, const unsigned long long *gcounts,
                               const RowGeom &g, const uint64_t *keys, uint64_t n, uint64_t *rows,
                               hipStream_t s);
hipError_t launch_fold_errcnt(const unsigned long long *gkeys, unsigned long long *errcnt,
                              uint64_t cap, unsigned long long *cms, uint32_t d, uint32_t w,
                              uint32_t shift, const uint64_t *seeds, uint64_t kinv, uint32_t dense,
                              hipStream_t s);
// binned-table path (spanagg_binned.hip)
hipError_t prepare_ingest_bt(size_t agg_lds);
size_t bt_agg2_lds_bytes(uint32_t log2sb, uint32_t grid);
// the binned launch's two kernels (the engine runs the aggregate on its own
// stream, beside the next launch's scatter)
hipError_t launch_bt_scatter(const IngestParams &P, hipStream_t s);
hipError_t launch_bt_aggregate(const IngestParams &P, hipStream_t s);
// its dense-index form (spanagg_dense.hip): the same launch pipeline
hipError_t prepare_ingest_dn(size_t agg_lds);
size_t dn_agg_lds_bytes(uint32_t log2sb, uint32_t grid);
hipError_t launch_dn_scatter(const IngestParams &P, hipStream_t s);
hipError_t launch_dn_aggregate(const IngestParams &P, hipStream_t s);
hipError_t launch_dn_bind(unsigned long long *gkeys, const uint64_t *index, const uint64_t *key_hash, uint64_t n,
                          uint32_t log2sb, hipStream_t s);
// range queries over the window ring (spanagg_range.hip): windows first ..
// first + n_win - 1 of a ring of n_windows slots (slot = window & (n_windows - 1)).
// hist [n_services][SA_HLL_HIST_BINS] (zeroed by the caller; nullptr: none): the
// max-merged registers holding each value; out [n_services][2^p] (nullptr:
// none): the merged registers themselves
hipError_t launch_range_merge(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p, uint64_t first,
                              uint32_t n_win, uint32_t *hist, uint8_t *out, hipStream_t s);
// the same for the n_sel services svc_map[0 .. n_sel) (device; nullptr: every
// service in id order, n_sel = n_services): row i of hist [n_sel][..] and out
// [n_sel][2^p] is service svc_map[i]; no other service's registers are read
hipError_t launch_range_merge_sel(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p,
                                  uint64_t first, uint32_t n_win, const uint32_t *svc_map, uint32_t n_sel,
                                  uint32_t *hist, uint8_t *out, hipStream_t s);
// sa_window_overlap's pair stage (spanagg_overlap.hip): pair_hist [n_sel (n_sel
// - 1) / 2][SA_HLL_HIST_BINS] (zeroed by the caller) = the value histogram of
// max(regs[i], regs[j]) for every i < j of regs [n_sel][2^p], pair index i *
// n_sel - i (i + 1) / 2 + (j - i - 1).  n_sel <= SA_OVERLAP_MAX_SERVICES.
// variant: 0, the product's counting; 1 and 2: the laboratory build's
// column-wise forms ("Service overlap over the window ring")
hipError_t launch_overlap_pairs(const uint8_t *regs, uint32_t n_sel, uint32_t p, uint32_t *pair_hist, uint32_t variant,
                                hipStream_t s);
// launch_fold_errcnt for the n_win windows from `first` in one launch
// (errcnt [n_windows][cap], cms [n_windows][slot_elems])
hipError_t launch_range_fold(const unsigned long long *gkeys, unsigned long long *errcnt, uint64_t cap,
                             unsigned long long *cms, uint64_t slot_elems, uint32_t d, uint32_t w, uint32_t shift,
                             const uint64_t *seeds, uint64_t kinv, uint32_t dense, uint32_t n_windows, uint64_t first,
                             uint32_t n_win, hipStream_t s);
// the same histogram of an already merged array [n_services][2^p]
hipError_t launch_hll_hist(const uint8_t *merged, uint32_t n_services, uint32_t p, uint32_t *hist, hipStream_t s);
// out [slot_elems] = the windows' count-min cells summed (zeroes out first)
hipError_t launch_range_cells(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t first,
                              uint32_t n_win, unsigned long long *out, hipStream_t s);
// out[i] = min over the d rows of cells[r][splitmix64(keys[i] ^ seeds[r]) >> shift]
hipError_t launch_range_query(const unsigned long long *cells, uint32_t d, uint32_t w, uint32_t shift,
                              const uint64_t *seeds, const uint64_t *keys, uint64_t n, unsigned long long *out,
                              hipStream_t s);
// sliding series over the ring (sa_window_series): output o of n_out covers
// the windows a + o .. a + o + width - 1.  hist [n_out][n_services][SA_HLL_HIST_BINS]
// (zeroed here): every output's max-merged registers counted by value
hipError_t launch_series_hll(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p, uint64_t a,
                             uint32_t width, uint32_t n_out, uint32_t *hist, hipStream_t s);
// out [n_out][n_keys] = range_query on the cells summed over each output's windows
hipError_t launch_series_query(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t a,
                               uint32_t width, uint32_t n_out, uint32_t d, uint32_t w, uint32_t shift,
                               const uint64_t *seeds, const uint64_t *keys, uint64_t n_keys, unsigned long long *out,
                               hipStream_t s);
// out [n_in] = count-min row 0 of each window a .. a + n_in - 1, summed
hipError_t launch_series_row0(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t a,
                              uint32_t n_in, uint32_t w, unsigned long long *out, hipStream_t s);
// heavy hitters over summed cells (sa_window_top; DESIGN.md section 4, "Heavy
// hitters over the window ring").  kTopCellsLds: the scan stages cells [d][w]
// in LDS up to this size -- 64 KiB, the default 4 x 2,048 sketch, two
// workgroups in a CU's 160 KiB -- and reads larger ones through global memory.
// kTopSel: pairs the final sort holds in one workgroup's LDS (16 B each).
constexpr uint32_t kTopCellsLds = 65536;
constexpr uint32_t kTopSel = 4096;  // = SA_TOP_MAX_K (asserted in spanagg_range.hip)
constexpr uint32_t kTopDigits = 16;  // bytes of (estimate, key): the select's launches
// The call's counters, the select's state and its output, on the device.
struct TopCtl {
  unsigned long long n_matched, n_resident, max_est, error_spans;  // (the host reads these four)
  unsigned long long pref_est, pref_nkey;  // the class's resolved digits (estimate, ~key), the others zero
  unsigned long long n_above, n_class;     // the gather's tickets
  uint32_t level, need, want, done, ticket, pad[3];
  uint32_t hist[256];
  ulonglong2 sel[kTopSel];  // the gather's pairs; the first `want` sorted, after the sort
};
// The whole query on `s`: gkeys [cap] scanned against cells [d][w] into cand
// [cap], then T->sel[0 .. min(k, T->n_matched)) = the first k matches by
// (estimate descending, key ascending).  k <= kTopSel, min_count >= 1.
hipError_t launch_top(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv, const unsigned long long *cells,
                      uint32_t d, uint32_t w, uint32_t shift, const uint64_t *seeds, uint32_t k,
                      unsigned long long min_count, ulonglong2 *cand, TopCtl *T, hipStream_t s);
// The select and the sort alone, for a scan of the caller's own: after it left
// its matches (x: what they are ranked by, y: the key; at most cap of them) in
// cand and T->n_matched, T->max_est (the largest x) and T->n_resident in a T
// whose first offsetof(TopCtl, sel) bytes were zeroed before it, T->sel[0 ..
// min(k, T->n_matched)) = the first k by (x descending, y ascending) and
// T->error_spans = the sum of row0[0 .. w).  row0 == nullptr with w == 0: no
// row to sum, T->error_spans stays 0 (the service-ranking scans, which take
// their spans themselves).  A key of 0 orders like any other.
hipError_t launch_top_select(const unsigned long long *row0, uint32_t w, uint32_t k, uint64_t cap,
                             const ulonglong2 *cand, TopCtl *T, hipStream_t s);
// movers between two ranges' summed cells (sa_window_movers; DESIGN.md section
// 4, "Movers between two ranges").  kMoversCellsLds: the scan stages both
// arrays in LDS while together they fit this size -- 128 KiB, two default
// sketches, one workgroup in a CU's 160 KiB -- and reads larger ones through
// global memory.
// (SA_MOVERS_CELLS_LDS: for A/B builds -- DESIGN.md has the measurement)
#ifndef SA_MOVERS_CELLS_LDS
#define SA_MOVERS_CELLS_LDS 131072
#endif
constexpr uint32_t kMoversCellsLds = SA_MOVERS_CELLS_LDS;
// What the call leaves beside TopCtl: the baseline range's row-0 sum and the
// selected rows' (baseline, current) estimates, in T->sel's order.
struct MoversOut {
  unsigned long long error_spans_base, pad;
  ulonglong2 est[kTopSel];
};
// The whole query on `s`: gkeys [cap] scanned against base and cur [d][w] with
// score = cur's estimate * nb - base's * nc (negated when fall != 0) into cand
// [cap], then T->sel[0 .. min(k, T->n_matched)) = the first k of the keys with
// score >= min_score as (score, key), by (score descending, key ascending),
// and O->est their estimates.  T->error_spans is cur's row-0 sum, T->max_est
// the largest score.  k <= kTopSel, 1 <= min_score.
hipError_t launch_movers(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv, const unsigned long long *base,
                         const unsigned long long *cur, uint32_t d, uint32_t w, uint32_t shift, const uint64_t *seeds,
                         uint64_t nb, uint64_t nc, uint32_t fall, uint32_t k, unsigned long long min_score,
                         ulonglong2 *cand, TopCtl *T, MoversOut *O, hipStream_t s);
// error onset over the window ring (sa_window_error_onset; spanagg_error_onset.hip;
// DESIGN.md section 4, "Error onset over the window ring").  A selected key's
// best split: t (the first window of "after", counted from the range's first)
// and the two sides' estimates B(t) and A(t).
struct ErrOnsetRow {
  unsigned long long t, before, after;
};
// What the call leaves beside TopCtl: the eligible keys and the selected rows'
// splits, in T->sel's order (96 KiB; the head and the first k rows are one copy).
struct ErrOnsetOut {
  unsigned long long n_eligible, pad;
  ErrOnsetRow row[kTopSel];
};
// The whole query on `s`: gkeys [cap] scanned against sum [d][w] -- the cells
// of the range's n_win windows summed -- and against the windows themselves,
// window j of the range at win_cells + ((first + j) & mask) * win_stride (the
// engine's ring: mask = n_windows - 1; an unwrapped [n_win][d * w] array: first
// 0, mask all ones).  Keys with E >= min_count are eligible (O->n_eligible);
// every eligible key's best split scored (fall 0 or 1) into cand [cap], then
// T->sel[0 .. min(k, T->n_matched)) = the first k of the keys with a best D >=
// min_score as (D, key), by (D descending, key ascending), and O->row their
// splits.  T->error_spans is sum's row-0 sum, T->max_est the largest D.  k <=
// kTopSel, 1 <= min_count, 1 <= min_score.  variant: 0, a lane a candidate;
// 1 (laboratory build only), a wave a candidate.
hipError_t launch_error_onset(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv,
                              const unsigned long long *sum, const unsigned long long *win_cells, uint64_t win_stride,
                              uint64_t first, uint64_t mask, uint32_t n_win, uint32_t d, uint32_t w, uint32_t shift,
                              const uint64_t *seeds, uint32_t fall, uint32_t k, unsigned long long min_count,
                              unsigned long long min_score, ulonglong2 *cand, TopCtl *T, ErrOnsetOut *O, uint32_t variant,
                              hipStream_t s);
// latency histograms over the window ring (spanagg_latency.hip; DESIGN.md
// section 4, "Latency histograms over the window ring"): ring [n_windows]
// [n_services][SA_LAT_BINS] u64.  Up to kLatLdsServices services a workgroup
// of the ingest kernel counts k_slots consecutive ring slots in dynamic LDS
// (1 KiB a service and slot); above, every span adds to the ring (k_slots 0).
// One workgroup of the LDS form a CU: its scalar registers (the launch
// parameters) leave room for 6 or 7 waves a SIMD, two 1,024-thread workgroups
// need 8; so it takes the slots that fit in 159 KiB of the CU's 160.  The HBM
// form has room for two.
constexpr uint32_t kLatLdsServices = 128;
struct LatGeom {
  uint32_t k_slots, per_cu;
};
inline LatGeom lat_geometry(uint32_t n_services, uint32_t n_windows) {
  if (n_services > kLatLdsServices) return {0, 2};
  const uint32_t fit = 159 / n_services;
  return {fit < n_windows ? fit : n_windows, 1};
}
hipError_t prepare_lat_ingest(size_t lds_bytes);
// One pass over P's start, end and meta columns beside the launch's ingest
// kernel (P: that kernel's parameters -- the same window fields, so both make
// the same in-ring decision): `grid` workgroups of `chunk` spans each (a
// multiple of 4, below 2^32).  k_slots: lat_geometry's, 0 = the HBM form.
hipError_t launch_lat_ingest(const IngestParams &P, unsigned long long *ring, uint32_t grid, uint64_t chunk,
                             uint32_t k_slots, hipStream_t s);
// sums [n_out][n_sel][SA_LAT_BINS]: output o = the rows of service sel[i]
// (device) summed over windows a + o .. a + o + width - 1
hipError_t launch_lat_sums(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows, const uint32_t *sel,
                           uint32_t n_sel, uint64_t a, uint32_t width, uint32_t n_out, unsigned long long *sums,
                           hipStream_t s);
// count [n_rows] and q_bin [n_rows][n_q] of sums [n_rows][SA_LAT_BINS]; q_ppm: host, n_q <= SA_LAT_MAX_Q
hipError_t launch_lat_scan(const unsigned long long *sums, uint64_t n_rows, const uint32_t *q_ppm, uint32_t n_q,
                           unsigned long long *count, uint8_t *q_bin, hipStream_t s);
// latency movers (sa_window_latency_movers; DESIGN.md section 4, "Latency
// movers over the window ring").  What the call leaves beside TopCtl: the
// two ranges' span counts, and per selected row (T->sel's order) the two
// counts and the two ranges' quantile bins, range 0 the baseline (128 KiB;
// the head and the first k rows are one copy).
struct LatMovRow {
  unsigned long long count[2];
  uint8_t q_bin[2][8];  // (SA_LAT_MAX_Q: asserted in spanagg_latency.hip)
};
struct LatMovOut {
  unsigned long long spans_base, spans_cur;
  LatMovRow row[kTopSel];
};
// Range sums over n_ranges in {1, 2}: sums [n_ranges][n_services][SA_LAT_BINS]
// = every service's rows summed over windows range[2r] .. range[2r + 1] (host;
// first and last, at most n_windows of them) -- the movers' baseline and
// current range, or the onset's one range for its pooled threshold.
hipError_t launch_lat_range_sums(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows,
                                 const uint64_t *range, uint32_t n_ranges, unsigned long long *sums, hipStream_t s);
// The rest of the query on `s`, from sums [2][n_services][SA_LAT_BINS]: every
// service scored by q_ppm[0] (min_count >= 1, min_shift >= 1, fall 0 or 1)
// into counts [2][n_services] and cand [n_services], the select and the sort
// -- T->sel[0 .. min(k, T->n_matched)) = (score, service) in the call's order,
// T->n_resident the eligible services -- and O: both ranges' spans and the
// selected rows' counts and bins of all n_q quantiles (q_ppm: host).  k <= kTopSel.
hipError_t launch_lat_movers(const unsigned long long *sums, uint32_t n_services, uint32_t k,
                             unsigned long long min_count, uint32_t min_shift, uint32_t fall, const uint32_t *q_ppm,
                             uint32_t n_q, unsigned long long *counts, ulonglong2 *cand, TopCtl *T, LatMovOut *O,
                             hipStream_t s);
// latency SLO burn (sa_window_slo; DESIGN.md section 4, "Latency SLO burn
// over sliding widths").  pairs [n_sel][n_cov][2] u64: covered window k =
// window a + k of the ring, service sel[i] (device; nullptr: service i, n_sel
// <= n_services): {its row's spans, those in bins above thr_bin[i] (device)}
hipError_t launch_slo_pairs(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows, const uint32_t *sel,
                            const uint8_t *thr_bin, uint32_t n_sel, uint64_t a, uint32_t n_cov,
                            unsigned long long *pairs, hipStream_t s);
// From pairs [n_sel][n_cov][2], n_cov = n_out + max(widths) - 1: total and slow
// [n_out][n_widths][n_sel], burning [n_out][n_sel] and alert [n_sel] as
// sa_slo_result's; prefix [n_sel][n_cov + 1][2] is scratch.  widths and
// limit_ppm: host, n_widths <= SA_SLO_MAX_WIDTHS; min_count >= 1.
hipError_t launch_slo_slide(const unsigned long long *pairs, uint32_t n_sel, uint32_t n_out, const uint32_t *widths,
                            const uint32_t *limit_ppm, uint32_t n_widths, unsigned long long min_count,
                            unsigned long long *prefix, unsigned long long *total, unsigned long long *slow,
                            uint8_t *burning, uint32_t *alert, hipStream_t s);
// latency onset (sa_window_latency_onset; DESIGN.md section 4, "Latency onset
// over the window ring").  A service's best split: t (the first window of
// "after", counted from the range's first; 0: no eligible split), the two
// sides' (total, slow) sums, and in a returned row its threshold bin.
struct OnsetRow {
  unsigned long long t, total_before, slow_before, total_after, slow_after, thr_bin;
};
// What the call leaves beside TopCtl: the range's spans and the selected rows
// in T->sel's order (192 KiB; the head and the first k rows are one copy).
struct OnsetOut {
  unsigned long long spans, pad;
  OnsetRow row[kTopSel];
};
// The pooled threshold's bins: thr_bin [n_services] = the bin of quantile q_ppm
// of each row of sums [n_services][SA_LAT_BINS] (launch_lat_range_sums over one
// range, a group's members' added up; sa_window_latency's rule).
hipError_t launch_onset_thr(const unsigned long long *sums, uint32_t n_services, uint32_t q_ppm, uint8_t *thr_bin,
                            hipStream_t s);
// The rest of the query on `s`, from pairs [n_sel][n_cov][2] (launch_slo_pairs
// over every service): every service's best split into rec [n_sel] and its
// candidate into cand [n_sel] (min_count >= 1, min_delta >= 1, fall 0 or 1),
// the select and the sort -- T->sel[0 .. min(k, T->n_matched)) = (delta_ppm <<
// 44 | min(count, 2^44 - 1), service) in the call's order, T->n_resident the
// eligible services -- and O: the range's spans and the selected rows with
// their threshold bins (thr_bin [n_sel], device; nullptr: 0).  k <= kTopSel.
hipError_t launch_onset(const unsigned long long *pairs, uint32_t n_sel, uint32_t n_cov, uint32_t k,
                        unsigned long long min_count, uint32_t min_delta, uint32_t fall, const uint8_t *thr_bin,
                        OnsetRow *rec, ulonglong2 *cand, TopCtl *T, OnsetOut *O, hipStream_t s);
// sorted union of series ids on the device (spanagg_union.hip): out = the
// distinct non-zero ids of in[0..n) ascending, *d_total (device u32) their
// count; scratch >= key_union_scratch_bytes(n); big_scratch / big_bytes: a
// grown-on-demand buffer for buckets the LDS sort cannot hold.  Synchronises
// `s` once (the largest bucket decides the sort's form).
size_t key_union_scratch_bytes(uint64_t n);
hipError_t key_union(const uint64_t *in, uint64_t n, uint64_t *out, uint32_t *d_total, void *scratch,
                     uint64_t **big_scratch, size_t *big_bytes, hipStream_t s);
// exponential histograms (spanagg_expo.hip)
hipError_t launch_expo_ingest(const ExpoParams &E, hipStream_t s);
hipError_t launch_expo_compact(const ExpoParams &E, unsigned long long *out_keys, ExpoRow *out_rows,
                               uint32_t *out_buckets, unsigned long long *out_n, hipStream_t s);
hipError_t launch_expo_init(ExpoHdr *hdr, int8_t *xscale, uint64_t cap, hipStream_t s);
size_t expo_count_lds_bytes(uint64_t cap, uint32_t max_size);
uint32_t expo_cached_entries(uint32_t max_size);  // the cached-probe kernel's cache entries (sa_debug_geometry)
// LDS entries of the slab counting kernel for one workgroup's LDS budget, and its LDS bytes
uint32_t expo_slab_entries(uint64_t cap, uint32_t max_size, size_t budget);
size_t expo_slab_lds_bytes(uint64_t cap, uint32_t max_size, uint32_t ne);
hipError_t prepare_expo_slab(size_t lds_bytes);
hipError_t prepare_expo_count(size_t lds_bytes);
hipError_t launch_expo_fast_probe(const uint64_t *d, const int32_t *scale, uint64_t n, double div, int32_t *fast,
                                  int32_t *exact, hipStream_t s);
hipError_t launch_log2_err_probe(uint32_t i0, uint32_t n, double *block_max, uint32_t blocks, hipStream_t s);
hipError_t launch_expo_probe(const double *v, const int32_t *scale, int32_t *idx_out, double *log_out, uint64_t n,
                             hipStream_t s);

}  // namespace sa
