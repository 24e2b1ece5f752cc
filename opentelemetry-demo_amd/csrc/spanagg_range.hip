// spanagg_range.hip -- range queries over the window ring (gfx950), for
// sa_window_range / sa_group_window_range (engine_read.cpp, spanagg_group.cpp):
// the sketches of the resident windows first..last merged on the device, so
// only the answers cross the bus.
//
//   range_fold_kernel    every window's per-slot ERROR counts into its cells
//                        (fold_errcnt_kernel over the range, one launch).
//   range_merge_kernel   HLL registers max-merged over the windows and the
//                        merged array's value histogram per service (the input
//                        of sa_hll_estimate_hist); the merged registers are
//                        stored only when a caller wants them.  Over one
//                        "window" it is the histogram of an already merged
//                        array (the group, after its all-reduce).
//                        With a service map it merges the selected services
//                        only (sa_window_overlap; the pairs: spanagg_overlap.hip).
//   range_cells_kernel   count-min cells summed over the windows (u64).
//   range_query_kernel   point queries on the summed cells, one thread a key.
//
// and for sa_window_series, the same answers for every trailing span of
// `width` windows in one pass over the ring:
//
//   series_hll_kernel    the sliding maximum of the registers by blocks of
//                        `width` windows and every output's histogram.
//   series_query_kernel  sliding sums of the keys' cells, their minimum per output.
//   series_row0_kernel   count-min row 0 summed per window (error_spans).
//
// and for sa_window_top / sa_group_window_top, the heaviest series of the
// summed cells among those resident in the key table:
//
//   top_scan_kernel      the key table against the cells: (estimate, key) of
//                        every match, the resident keys, the largest estimate
//                        (sa_device.h's table_scan, the estimate as its score).
//   top_prepare_kernel   error_spans (a caller without a row to sum: 0) and
//                        the select's first state.
//   top_digit_kernel     one digit of the radix select over (estimate, ~key),
//                        chosen on the device.
//   top_gather_kernel    the selected pairs and the threshold's class.
//   top_sort_kernel      their order, in one workgroup's LDS.
//
// and for sa_window_movers / sa_group_window_movers, the series whose ERROR
// rate changed most between two ranges, with the same select and sort:
//
//   movers_scan_kernel   the key table against both ranges' cells: (score,
//                        key) of every match, the resident keys, the largest
//                        score (table_scan again).
//   movers_rows_kernel   the selected keys' estimates in both ranges, and the
//                        baseline's error_spans.
//
// Every result is an integer maximum or an integer sum, so the order of the
// atomics does not show: two calls, and one engine against a group, give the
// same bits.
#include <algorithm>
#include <cstddef>

#include "sa_device.h"
#include "spanagg.h"

namespace sa {
namespace {

constexpr uint32_t kRangeBlock = 256;  // four waves: each walks a quarter of the windows
constexpr uint32_t kRangeWaves = kRangeBlock / 64;
constexpr uint32_t kRangeBins = SA_HLL_HIST_BINS;
// windows whose 16-B loads a thread issues before it takes their maxima (the
// walk is one dependent chain per thread otherwise)
// (SA_RANGE_IN_FLIGHT: for A/B builds -- DESIGN.md has the measurement)
#ifndef SA_RANGE_IN_FLIGHT
#define SA_RANGE_IN_FLIGHT 8
#endif
constexpr uint32_t kRangeInFlight = SA_RANGE_IN_FLIGHT;
constexpr uint32_t kCellsInFlight = 4;
constexpr uint32_t kCellChunks = 16;  // the cell sum's window chunks (blockIdx.y)

// Workgroup b serves service b / wgs and strides the service's tiles of 64
// threads; a thread owns 16 consecutive registers (tps = 2^log2tps threads a
// service, 2^p = 16 tps).  The workgroup's four waves each walk a quarter of
// the windows for the same tile -- a 512 MB ring of 32 services is 512 tiles,
// two waves a CU if a tile were one wave's -- and their partial maxima meet
// in LDS; wave 0 stores and counts.  regs: [win_mask + 1][n_services][2^p].
// hist (nullptr: none) [n_services][64] must be zero; out (nullptr: none)
// [n_services][2^p].  svc_map (nullptr: every service, in id order): row b /
// wgs of hist and out is service svc_map[b / wgs] of the ring -- the selected
// services of sa_window_overlap, in the caller's order; the others are not read.
__global__ __launch_bounds__(kRangeBlock) void range_merge_kernel(const uint4 *regs, uint64_t slot16, uint32_t win_mask,
                                                                  uint64_t first, uint32_t n_win, uint32_t log2tps,
                                                                  uint32_t wgs, const uint32_t *svc_map, uint32_t *hist,
                                                                  uint4 *out) {
  __shared__ uint32_t h[kRangeBins];  // wave 0's histogram
  __shared__ uint4 part[kRangeWaves - 1][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kRangeBins) h[threadIdx.x] = 0;  // (ordered before the first count by the loop's barrier)
  const uint32_t svc = blockIdx.x / wgs, wg = blockIdx.x % wgs, tps = 1u << log2tps;
  const uint32_t src = svc_map ? svc_map[svc] : svc;  // the ring's row; svc: the output's
  const uint32_t per = (n_win + kRangeWaves - 1) / kRangeWaves;
  const uint32_t k0 = min(n_win, wave * per), k1 = min(n_win, k0 + per);
  for (uint32_t t = wg; t < (tps + 63) / 64; t += wgs) {  // (the same trips for every thread)
    const uint32_t c = t * 64 + lane;
    const uint64_t at = ((uint64_t)src << log2tps) + c;
    uint4 acc{0, 0, 0, 0};
    if (c < tps) {
      uint32_t k = k0;
      for (; k + kRangeInFlight <= k1; k += kRangeInFlight) {
        uint4 v[kRangeInFlight];
#pragma unroll
        for (uint32_t j = 0; j < kRangeInFlight; ++j) v[j] = regs[((first + k + j) & win_mask) * slot16 + at];
#pragma unroll
        for (uint32_t j = 0; j < kRangeInFlight; ++j) acc = max_u8x16(acc, v[j]);
      }
      for (; k < k1; ++k) acc = max_u8x16(acc, regs[((first + k) & win_mask) * slot16 + at]);
    }
    if (wave) part[wave - 1][lane] = acc;
    __syncthreads();
    if (wave == 0 && c < tps) {
#pragma unroll
      for (uint32_t w = 0; w < kRangeWaves - 1; ++w) acc = max_u8x16(acc, part[w][lane]);
      if (out) out[((uint64_t)svc << log2tps) + c] = acc;
      if (hist) {
        const uint32_t w4[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
        for (uint32_t j = 0; j < 16; ++j) {
          const uint32_t v = (w4[j >> 2] >> (8 * (j & 3))) & 0xFFu;
          atomicAdd(&h[v < kRangeBins ? v : kRangeBins - 1], 1u);
        }
      }
    }
    __syncthreads();  // (the partial maxima are read before the next tile's)
  }
  if (hist && threadIdx.x < kRangeBins && h[threadIdx.x])
    atomicAdd(hist + (uint64_t)svc * kRangeBins + threadIdx.x, h[threadIdx.x]);
}

// fold_errcnt_kernel for every window of the range in one launch: workgroup
// row y folds window first + y (errcnt [W][cap], cms [W][slot_elems])
__global__ __launch_bounds__(256) void range_fold_kernel(const unsigned long long *gkeys, unsigned long long *errcnt,
                                                         uint64_t cap, unsigned long long *cms, uint64_t slot_elems,
                                                         uint32_t d, uint32_t w, uint32_t shift, const uint64_t *seeds,
                                                         uint64_t kinv, uint32_t dense, uint32_t win_mask,
                                                         uint64_t first) {
  const uint64_t ws = (first + blockIdx.y) & win_mask;
  fold_errcnt_slots(gkeys, errcnt + ws * cap, cap, cms + ws * slot_elems, d, w, shift, seeds, kinv, dense);
}

// out[i] += sum of cells[w][i] over this workgroup row's chunk of the windows
// (out zeroed first; u64 adds)
__global__ __launch_bounds__(256) void range_cells_kernel(const unsigned long long *cells, uint64_t slot_elems,
                                                          uint32_t win_mask, uint64_t first, uint32_t n_win,
                                                          uint32_t per_chunk, unsigned long long *out) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= slot_elems) return;
  const uint32_t k0 = blockIdx.y * per_chunk, k1 = min(n_win, k0 + per_chunk);
  unsigned long long acc = 0;
  uint32_t k = k0;
  for (; k + kCellsInFlight <= k1; k += kCellsInFlight) {
    unsigned long long v[kCellsInFlight];
#pragma unroll
    for (uint32_t j = 0; j < kCellsInFlight; ++j) v[j] = cells[((first + k + j) & win_mask) * slot_elems + i];
#pragma unroll
    for (uint32_t j = 0; j < kCellsInFlight; ++j) acc += v[j];
  }
  for (; k < k1; ++k) acc += cells[((first + k) & win_mask) * slot_elems + i];
  if (acc) atomicAdd(out + i, acc);
}

// out[i] = min over the rows of cells[r][splitmix64(keys[i] ^ seeds[r]) >> shift]
__global__ __launch_bounds__(256) void range_query_kernel(const unsigned long long *cells, uint32_t d, uint32_t w,
                                                          uint32_t shift, const uint64_t *seeds, const uint64_t *keys,
                                                          uint64_t n, unsigned long long *out) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t key = keys[i];
    unsigned long long m = ~0ULL;
    for (uint32_t r = 0; r < d; ++r) {
      const uint64_t col = splitmix64(key ^ seeds[r]) >> shift;  // < w: shift = 64 - log2 w, w >= 2
      const unsigned long long v = cells[(uint64_t)r * w + col];
      m = v < m ? v : m;
    }
    out[i] = m;
  }
}

// ---- sliding series (sa_window_series): output o of n_out covers the windows
// a + o .. a + o + width - 1 of the ring ----
constexpr uint32_t kSeriesLanes = 64;          // one wave a workgroup: the walk is one chain per column
constexpr uint32_t kSeriesStashBytes = 32768;  // LDS stash of a workgroup (the bound on width)
constexpr uint32_t kSeriesChunk1 = 16;         // width 1: outputs a workgroup takes
// A tile inside one service counts into 8 copies of the 64 bins, by lane & 7:
// most registers hold one of a few values, and 64 lanes on one LDS word take
// turns.  68 words a copy: a bin's copies lie in different banks.
constexpr uint32_t kSeriesCopies = 8, kSeriesCopyWords = 68;

__device__ __forceinline__ uint32_t series_hist_words(uint32_t nsv) {
  return nsv == 1 ? kSeriesCopies * kSeriesCopyWords : nsv * kRangeBins;
}

// One output's registers m (16 a thread that is `on`) counted into the LDS
// histogram h (zero before and after), then one atomicAdd per non-zero bin
// into out = hist[output][svc0]; nsv: services of the tile.
__device__ __forceinline__ void series_count(uint4 m, bool on, uint32_t *h, uint32_t hbase, uint32_t nsv,
                                             uint32_t lane, uint32_t *out, uint32_t svc0, uint32_t n_services) {
  if (on) {
    const uint32_t w4[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
    for (uint32_t b = 0; b < 16; ++b) {
      const uint32_t x = (w4[b >> 2] >> (8 * (b & 3))) & 0xFFu;
      atomicAdd(&h[hbase + (x < kRangeBins ? x : kRangeBins - 1)], 1u);
    }
  }
  __syncthreads();
  if (nsv == 1) {  // (64 lanes, 64 bins)
    uint32_t n = 0;
#pragma unroll
    for (uint32_t cp = 0; cp < kSeriesCopies; ++cp) {
      n += h[cp * kSeriesCopyWords + lane];
      h[cp * kSeriesCopyWords + lane] = 0;
    }
    if (n) atomicAdd(out + lane, n);
  } else {
    for (uint32_t i = lane; i < nsv * kRangeBins; i += kSeriesLanes) {
      const uint32_t n = h[i];
      if (n && svc0 + i / kRangeBins < n_services) atomicAdd(out + i, n);
      h[i] = 0;
    }
  }
  __syncthreads();
}

// Sliding maximum by blocks of `width` windows (van Herk / Gil-Werman).  The
// window slot is S * tps columns of 16 registers; a workgroup takes one tile
// of L consecutive columns (L a power of two <= 64: a tile lies in one
// service or covers L / tps whole ones) and one block j of `width` windows.
//   backward  block j from its end to its start: the running suffix maximum
//             of step r goes to stash[r] (LDS, [width][L] uint4)
//   forward   block j + 1 from its start with the running prefix maximum P
//             (zero before the first step): output j * width + r has the
//             registers max(stash[r], P before step r)
// so a window's registers are read twice.  A block whose stash would pass
// kSeriesStashBytes goes chunk by chunk (chunk < width steps): a first walk
// over block j leaves later[c], the maximum of the chunks after c; then for
// each chunk in turn the backward walk fills the stash with the suffix
// maxima inside the chunk, and step r's suffix maximum is max(stash[r - chunk
// start], later[c]).  The stash holds chunk + width / chunk entries and block
// j is read twice: three reads a window.  At width 1 every window is its own
// output: no stash, one read, kSeriesChunk1 outputs a workgroup.  Every
// output's registers are counted into an LDS histogram per service of the
// tile and leave as one atomicAdd per non-zero bin.  hist
// [n_out][n_services][64] must be zero.  Grid: tiles * blocks.
__global__ __launch_bounds__(kSeriesLanes) void series_hll_kernel(const uint4 *regs, uint64_t slot16, uint32_t win_mask,
                                                                  uint64_t a, uint32_t width, uint32_t n_out,
                                                                  uint32_t log2tps, uint32_t n_services, uint32_t L,
                                                                  uint32_t chunk, uint32_t tiles, uint32_t *hist) {
  extern __shared__ uint4 series_lds[];
  const uint32_t lane = threadIdx.x;
  const uint32_t nsv = max(1u, L >> log2tps);  // services of a tile
  const uint32_t C = (width + chunk - 1) / chunk;  // chunks of a block (1: the whole block in the stash)
  uint4 *stash = series_lds;                       // [chunk][L] (none at width 1)
  uint4 *later = stash + (size_t)chunk * L;        // [C][L] (none when C == 1)
  uint32_t *h = reinterpret_cast<uint32_t *>(series_lds + (width == 1 ? 0 : (size_t)(chunk + (C > 1 ? C : 0)) * L));
  for (uint32_t i = lane; i < series_hist_words(nsv); i += kSeriesLanes) h[i] = 0;
  const uint32_t tile = blockIdx.x % tiles, j = blockIdx.x / tiles;
  const uint64_t c = (uint64_t)tile * L + lane;  // the thread's column of the slot
  const bool on = lane < L && c < slot16;
  const uint32_t svc0 = (uint32_t)(((uint64_t)tile * L) >> log2tps);  // the tile's first service
  const uint32_t hbase = nsv == 1 ? (lane & (kSeriesCopies - 1)) * kSeriesCopyWords : (lane >> log2tps) * kRangeBins;

  if (width == 1) {
    const uint32_t o0 = j * kSeriesChunk1, R = min(kSeriesChunk1, n_out - o0);
    __syncthreads();  // (the zeroed histogram)
    for (uint32_t r0 = 0; r0 < R; r0 += kRangeInFlight) {  // (the same trips for every thread)
      uint4 v[kRangeInFlight];
#pragma unroll
      for (uint32_t k = 0; k < kRangeInFlight; ++k) {
        v[k] = uint4{0, 0, 0, 0};
        if (on && r0 + k < R) v[k] = regs[((a + o0 + r0 + k) & win_mask) * slot16 + c];
      }
#pragma unroll
      for (uint32_t k = 0; k < kRangeInFlight; ++k) {
        if (r0 + k >= R) break;  // (uniform)
        series_count(v[k], on, h, hbase, nsv, lane, hist + ((uint64_t)(o0 + r0 + k) * n_services + svc0) * kRangeBins,
                     svc0, n_services);
      }
    }
    return;
  }

  const uint32_t o0 = j * width;                // the block's first output, and its first window past a
  const uint32_t R = min(width, n_out - o0);    // outputs of this block
  const uint64_t w0 = a + o0, w1 = w0 + width;  // first windows of block j and of block j + 1
  if (on && C > 1) {  // later[c] = the maximum of block j's chunks after c
    uint4 run{0, 0, 0, 0};
    for (uint32_t cc = C; cc-- > 0;) {
      later[(size_t)cc * L + lane] = run;
      const uint32_t lo = cc * chunk, hi = min(width, lo + chunk);
      uint32_t r = lo;
      for (; r + kRangeInFlight <= hi; r += kRangeInFlight) {
        uint4 v[kRangeInFlight];
#pragma unroll
        for (uint32_t k = 0; k < kRangeInFlight; ++k) v[k] = regs[((w0 + r + k) & win_mask) * slot16 + c];
#pragma unroll
        for (uint32_t k = 0; k < kRangeInFlight; ++k) run = max_u8x16(run, v[k]);
      }
      for (; r < hi; ++r) run = max_u8x16(run, regs[((w0 + r) & win_mask) * slot16 + c]);
    }
  }
  __syncthreads();  // (the zeroed histogram; a thread reads only its own stash and later column)

  uint4 P{0, 0, 0, 0};
  for (uint32_t cc = 0; cc < C && cc * chunk < R; ++cc) {  // (the same trips for every thread)
    const uint32_t lo = cc * chunk, hi = min(width, lo + chunk), end = min(hi, R);
    uint4 E{0, 0, 0, 0};
    if (on) {  // backward: steps hi - 1 .. lo
      uint4 acc{0, 0, 0, 0};
      uint32_t r = hi;
      for (; r >= lo + kRangeInFlight; r -= kRangeInFlight) {
        uint4 v[kRangeInFlight];
#pragma unroll
        for (uint32_t k = 0; k < kRangeInFlight; ++k) v[k] = regs[((w0 + r - 1 - k) & win_mask) * slot16 + c];
#pragma unroll
        for (uint32_t k = 0; k < kRangeInFlight; ++k) {
          acc = max_u8x16(acc, v[k]);
          stash[(size_t)(r - 1 - k - lo) * L + lane] = acc;
        }
      }
      for (; r > lo; --r) {
        acc = max_u8x16(acc, regs[((w0 + r - 1) & win_mask) * slot16 + c]);
        stash[(size_t)(r - 1 - lo) * L + lane] = acc;
      }
      if (C > 1) E = later[(size_t)cc * L + lane];
    }
    for (uint32_t r0 = lo; r0 < end; r0 += kRangeInFlight) {
      uint4 v[kRangeInFlight];
#pragma unroll
      for (uint32_t k = 0; k < kRangeInFlight; ++k) {
        // step r's window of block j + 1 is needed by the outputs after r only
        v[k] = uint4{0, 0, 0, 0};
        if (on && r0 + k < end && r0 + k + 1 < R) v[k] = regs[((w1 + r0 + k) & win_mask) * slot16 + c];
      }
#pragma unroll
      for (uint32_t k = 0; k < kRangeInFlight; ++k) {
        const uint32_t r = r0 + k;
        if (r >= end) break;  // (uniform)
        uint4 m{0, 0, 0, 0};
        if (on) {
          m = max_u8x16(max_u8x16(stash[(size_t)(r - lo) * L + lane], E), P);
          P = max_u8x16(P, v[k]);
        }
        series_count(m, on, h, hbase, nsv, lane, hist + ((uint64_t)(o0 + r) * n_services + svc0) * kRangeBins, svc0,
                     n_services);
      }
    }
  }
}

// Point queries of every output: thread (key i, chunk blockIdx.y of the
// outputs) seeds d running sums with the `width` covered cells at the key's d
// columns, then adds the entering window's cell and takes off the leaving
// one's per output (u64, exact).  out [n_out][n_keys].
__global__ __launch_bounds__(256) void series_query_kernel(const unsigned long long *cms, uint64_t slot_elems,
                                                           uint32_t win_mask, uint64_t a, uint32_t width,
                                                           uint32_t n_out, uint32_t per_chunk, uint32_t d, uint32_t w,
                                                           uint32_t shift, const uint64_t *seeds, const uint64_t *keys,
                                                           uint64_t n_keys, unsigned long long *out) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n_keys) return;
  const uint32_t o0 = blockIdx.y * per_chunk, o1 = min(n_out, o0 + per_chunk);
  const uint64_t key = keys[i];
  uint64_t at[8];  // (cms_d <= 8) the key's cell of each row within a slot
  unsigned long long sum[8];
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) {
    at[r] = r < d ? (uint64_t)r * w + (splitmix64(key ^ seeds[r]) >> shift) : 0;  // col < w: shift = 64 - log2 w
    sum[r] = 0;
  }
#pragma unroll 4
  for (uint32_t k = 0; k < width; ++k) {
    const unsigned long long *slot = cms + ((a + o0 + k) & win_mask) * slot_elems;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
      if (r < d) sum[r] += slot[at[r]];
  }
  for (uint32_t o = o0; o < o1; ++o) {
    if (o > o0) {
      const unsigned long long *in = cms + ((a + o + width - 1) & win_mask) * slot_elems;
      const unsigned long long *gone = cms + ((a + o - 1) & win_mask) * slot_elems;
#pragma unroll
      for (uint32_t r = 0; r < 8; ++r)
        if (r < d) sum[r] += in[at[r]] - gone[at[r]];
    }
    unsigned long long m = ~0ULL;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r)
      if (r < d) m = sum[r] < m ? sum[r] : m;
    out[(uint64_t)o * n_keys + i] = m;
  }
}

// out[k] = the sum of count-min row 0 of window a + k (every ERROR span the
// window's sketch counted, once); one workgroup a window
__global__ __launch_bounds__(256) void series_row0_kernel(const unsigned long long *cms, uint64_t slot_elems,
                                                          uint32_t win_mask, uint64_t a, uint32_t w,
                                                          unsigned long long *out) {
  __shared__ unsigned long long part[256];
  const unsigned long long *row = cms + ((a + blockIdx.x) & win_mask) * slot_elems;
  unsigned long long acc = 0;
  for (uint32_t i = threadIdx.x; i < w; i += 256) acc += row[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = part[0];
}

// ---- heavy hitters (sa_window_top): the key table scanned against the summed
// cells, the first k of (estimate descending, key ascending) selected ----
constexpr uint32_t kTopScanBlock = 1024;  // 16 waves: two workgroups of 64 KiB of cells fill a CU's 32
constexpr uint32_t kTopBlock = 256;       // the select's digit and gather kernels
constexpr uint32_t kTopSortBlock = 1024;
static_assert(kTopSel == SA_TOP_MAX_K, "the sort holds the largest k");
static_assert(kMoversCellsLds <= 160 * 1024, "a workgroup's LDS");

// A candidate is the pair (estimate, key), ordered by estimate descending then
// key ascending: as a 128-bit number (estimate, ~key) the largest comes first.
// Its 16 bytes are the select's digits, 15 (the estimate's top byte) .. 0 (~key's
// lowest).  top_high: the digits >= level kept, those below cleared.
__device__ __forceinline__ void top_high(unsigned long long est, unsigned long long nkey, uint32_t level,
                                         unsigned long long &he, unsigned long long &hk) {
  if (level >= 16) {
    he = 0, hk = 0;
  } else if (level >= 8) {
    const uint32_t sh = 8 * (level - 8);
    he = (est >> sh) << sh, hk = 0;
  } else {
    const uint32_t sh = 8 * level;
    he = est, hk = (nkey >> sh) << sh;
  }
}
__device__ __forceinline__ uint32_t top_digit(unsigned long long est, unsigned long long nkey, uint32_t level) {
  return (uint32_t)((level >= 8 ? est >> (8 * (level - 8)) : nkey >> (8 * level)) & 0xFFu);
}

// table_scan (sa_device.h) with a key's estimate as its score: the minimum
// over the rows of cells [d][w] -- staged in LDS (LDS = 1: d * w * 8 <=
// kTopCellsLds dynamic bytes) or read through global memory.  Keys with an
// estimate >= min_count (>= 1) match.
template <int LDS>
__global__ __launch_bounds__(kTopScanBlock) void top_scan_kernel(const unsigned long long *gkeys, uint64_t cap,
                                                                 uint64_t kinv, const unsigned long long *cells,
                                                                 uint32_t d, uint32_t w, uint32_t shift,
                                                                 const uint64_t *seeds, unsigned long long min_count,
                                                                 ulonglong2 *cand, TopCtl *T) {
  extern __shared__ unsigned long long top_cells[];
  const unsigned long long *c = cells;
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < d * w; i += kTopScanBlock) top_cells[i] = cells[i];
    __syncthreads();
    c = top_cells;
  }
  uint64_t sd[8];  // (cms_d <= 8)
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
  table_scan<kTopScanBlock>(gkeys, cap, kinv, cand, T, [&](uint64_t key, unsigned long long &est) {
    est = ~0ULL;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
      if (r < d) {
        const uint64_t col = splitmix64(key ^ sd[r]) >> shift;  // < w: shift = 64 - log2 w, w >= 2
        const unsigned long long v = c[(uint64_t)r * w + col];
        est = v < est ? v : est;
      }
    }
    return est >= min_count;
  });
}

// After the scan (one workgroup): error_spans = the sum of row0 [w], row 0 of
// the cells (a scan with no row to sum passes w = 0: the loop never runs, so a
// null row0 is not read), and the select's first state.  At most kTopSel matches: nothing to
// select (level 16: no digit resolved, every match is in the class).
// Otherwise the first digit is the top non-zero byte of the largest estimate.
__global__ __launch_bounds__(kTopBlock) void top_prepare_kernel(const unsigned long long *row0, uint32_t w, uint32_t k,
                                                                TopCtl *T) {
  __shared__ unsigned long long part[kTopBlock];
  unsigned long long acc = 0;
  for (uint32_t i = threadIdx.x; i < w; i += kTopBlock) acc += row0[i];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t s = kTopBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x) return;
  T->error_spans = part[0];
  const unsigned long long n = T->n_matched;
  const uint32_t want = (uint32_t)(n < k ? n : k);
  T->want = want, T->need = want;
  T->pref_est = 0, T->pref_nkey = 0;
  T->done = n <= kTopSel ? 1u : 0u;
  T->level = n <= kTopSel ? 16u : 8u + (63u - (uint32_t)__clzll((long long)T->max_est)) / 8u;
}

// One digit of the radix select, chosen on the device.  The class is the
// matches whose digits above T->level equal the prefix; `need` of the class's
// largest are still to be found.  Every workgroup counts its stripe of the
// class by the digit at T->level (LDS, then one atomic per non-zero bin); the
// last one to finish walks the bins from 255 down to the bin b the need-th
// largest falls in: the bins above b are selected whole, b joins the prefix,
// need shrinks by what was above.  Done once the selected matches and the new
// class fit the sort (kTopSel) or digit 0 is resolved; a launch after that
// returns at once.  T->hist and T->ticket are zero between launches.
__global__ __launch_bounds__(kTopBlock) void top_digit_kernel(const ulonglong2 *cand, TopCtl *T) {
  __shared__ uint32_t h[256];
  __shared__ uint32_t last;
  if (T->done) return;  // (every workgroup reads the state before the last one changes it)
  const uint32_t level = T->level;
  const unsigned long long pe = T->pref_est, pk = T->pref_nkey, n = T->n_matched;
  h[threadIdx.x] = 0;
  __syncthreads();
  for (uint64_t i = blockIdx.x * (uint64_t)kTopBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kTopBlock) {
    const ulonglong2 c = cand[i];
    unsigned long long he, hk;
    top_high(c.x, ~c.y, level + 1, he, hk);
    if (he != pe || hk != pk) continue;
    // ties put a whole wave on one bin: the lanes that share the first lane's
    // digit leave as one add, the others one by one
    const uint32_t dg = top_digit(c.x, ~c.y, level);
    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg);
    const uint64_t same = __ballot(dg == d0);
    if (dg != d0)
      atomicAdd(&h[dg], 1u);
    else if (lane_rank(same) == 0)
      atomicAdd(&h[d0], (uint32_t)__popcll(same));
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&T->hist[threadIdx.x], h[threadIdx.x]);
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(&T->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!last) return;
  __threadfence();
  h[threadIdx.x] = __hip_atomic_load(&T->hist[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  T->hist[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x) return;
  T->ticket = 0;
  uint32_t need = T->need, above = 0, b = 255;
  for (;; --b) {  // (the class holds at least `need`: some bin reaches it)
    if (above + h[b] >= need || b == 0) break;
    above += h[b];
  }
  need -= above;
  T->need = need;
  if (level >= 8)
    T->pref_est = pe | ((unsigned long long)b << (8 * (level - 8)));
  else
    T->pref_nkey = pk | ((unsigned long long)b << (8 * level));
  if (level == 0 || (unsigned long long)(T->want - need) + h[b] <= kTopSel)
    T->done = 1;
  else
    T->level = level - 1;
}

// The matches above the class (digits >= T->level greater than the prefix)
// into T->sel from the front, the class itself from the back; a class member
// that would meet the front is dropped (only when digit 0 left equal pairs:
// they are interchangeable).
__global__ __launch_bounds__(kTopBlock) void top_gather_kernel(const ulonglong2 *cand, TopCtl *T) {
  const uint32_t level = T->level;
  const unsigned long long pe = T->pref_est, pk = T->pref_nkey, n = T->n_matched;
  const unsigned long long room = kTopSel - (T->want - T->need);  // the class's share of sel
  for (uint64_t i = blockIdx.x * (uint64_t)kTopBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kTopBlock) {
    const ulonglong2 c = cand[i];
    unsigned long long he, hk;
    top_high(c.x, ~c.y, level, he, hk);
    const bool above = he > pe || (he == pe && hk > pk), in_class = he == pe && hk == pk;
    if (above) {
      const unsigned long long pos = wave_ticket(&T->n_above, __ballot(true));
      if (pos < kTopSel) T->sel[pos] = c;
    } else if (in_class) {
      const unsigned long long pos = wave_ticket(&T->n_class, __ballot(true));
      if (pos < room) T->sel[kTopSel - 1 - pos] = c;
    }
  }
}

// One workgroup: T->sel's two ends into LDS, padded to a power of two with
// pairs that sort last, a bitonic sort by (estimate descending, key
// ascending), and the first T->want back to the front of T->sel.
__global__ __launch_bounds__(kTopSortBlock) void top_sort_kernel(TopCtl *T) {
  extern __shared__ ulonglong2 top_sel[];  // [kTopSel]
  const uint32_t na = (uint32_t)min(T->n_above, (unsigned long long)kTopSel);
  const uint32_t nc = (uint32_t)min(T->n_class, (unsigned long long)(kTopSel - na));
  const uint32_t n = na + nc, want = min(T->want, n);
  uint32_t P = 64;
  while (P < n) P <<= 1;
  for (uint32_t i = threadIdx.x; i < P; i += kTopSortBlock)
    top_sel[i] = i < na ? T->sel[i] : i < n ? T->sel[kTopSel - 1 - (i - na)] : ulonglong2{0ULL, ~0ULL};
  __syncthreads();
  for (uint32_t k2 = 2; k2 <= P; k2 <<= 1) {
    for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
      for (uint32_t i = threadIdx.x; i < P; i += kTopSortBlock) {
        const uint32_t o = i ^ j;
        if (o > i) {
          const ulonglong2 a = top_sel[i], b = top_sel[o];
          const bool b_first = b.x > a.x || (b.x == a.x && b.y < a.y);
          if (b_first == ((i & k2) == 0)) top_sel[i] = b, top_sel[o] = a;
        }
      }
      __syncthreads();
    }
  }
  for (uint32_t i = threadIdx.x; i < want; i += kTopSortBlock) T->sel[i] = top_sel[i];
}

// ---- movers (sa_window_movers): the key table scanned against two ranges'
// summed cells at once, ranked by the change; the select and the sort are the
// heavy hitters' ----
// The key's estimates in base and cur [d][w]: its d columns are computed once
// and read in both (range_query_kernel's arithmetic, twice).
__device__ __forceinline__ void movers_estimates(const unsigned long long *base, const unsigned long long *cur,
                                                 uint32_t d, uint32_t w, uint32_t shift, const uint64_t (&sd)[8],
                                                 uint64_t key, unsigned long long &eb, unsigned long long &ec) {
  eb = ~0ULL, ec = ~0ULL;
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) {  // (cms_d <= 8)
    if (r < d) {
      const uint64_t at = (uint64_t)r * w + (splitmix64(key ^ sd[r]) >> shift);  // col < w: shift = 64 - log2 w, w >= 2
      const unsigned long long vb = base[at], vc = cur[at];
      eb = vb < eb ? vb : eb;
      ec = vc < ec ? vc : ec;
    }
  }
}

// top_scan_kernel over two arrays: a key's estimates eb and ec taken from base
// and cur -- both staged in LDS (LDS = 1: 2 * d * w * 8 <= kMoversCellsLds
// dynamic bytes, base first) or both read through global memory -- and score =
// ec * nb - eb * nc as a signed number, negated when `fall`.  Keys with score
// >= min_score (>= 1, so the score orders as an unsigned number) match.
template <int LDS>
__global__ __launch_bounds__(kTopScanBlock) void movers_scan_kernel(const unsigned long long *gkeys, uint64_t cap,
                                                                    uint64_t kinv, const unsigned long long *base,
                                                                    const unsigned long long *cur, uint32_t d,
                                                                    uint32_t w, uint32_t shift, const uint64_t *seeds,
                                                                    unsigned long long nb, unsigned long long nc,
                                                                    uint32_t fall, unsigned long long min_score,
                                                                    ulonglong2 *cand, TopCtl *T) {
  extern __shared__ unsigned long long movers_cells[];  // [2][d][w]
  const unsigned long long *b = base, *c = cur;
  if constexpr (LDS) {
    const uint32_t n = d * w;
    for (uint32_t i = threadIdx.x; i < n; i += kTopScanBlock) movers_cells[i] = base[i], movers_cells[n + i] = cur[i];
    __syncthreads();
    b = movers_cells, c = movers_cells + n;
  }
  uint64_t sd[8];  // (cms_d <= 8)
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
  table_scan<kTopScanBlock>(gkeys, cap, kinv, cand, T, [&](uint64_t key, unsigned long long &score) {
    unsigned long long eb, ec;
    movers_estimates(b, c, d, w, shift, sd, key, eb, ec);
    score = ec * nb - eb * nc;  // (two's complement: the signed difference)
    if (fall) score = 0ULL - score;
    return (long long)score >= 1 && score >= min_score;
  });
}

// After the sort: O->est[i] = the (baseline, current) estimates of row i of
// T->sel, i < T->want (<= kTopSel), from the same arrays the scan read; and,
// by workgroup 0, O->error_spans_base = the sum of row 0 of base (cur's is
// top_prepare_kernel's T->error_spans).
__global__ __launch_bounds__(kTopBlock) void movers_rows_kernel(const unsigned long long *base,
                                                                const unsigned long long *cur, uint32_t d, uint32_t w,
                                                                uint32_t shift, const uint64_t *seeds, const TopCtl *T,
                                                                MoversOut *O) {
  __shared__ unsigned long long part[kTopBlock];
  const uint32_t i = blockIdx.x * kTopBlock + threadIdx.x;
  if (i < T->want && i < kTopSel) {
    uint64_t sd[8];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
    unsigned long long eb, ec;
    movers_estimates(base, cur, d, w, shift, sd, T->sel[i].y, eb, ec);
    O->est[i] = ulonglong2{eb, ec};
  }
  if (blockIdx.x) return;
  unsigned long long acc = 0;
  for (uint32_t j = threadIdx.x; j < w; j += kTopBlock) acc += base[j];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (uint32_t s = kTopBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) O->error_spans_base = part[0], O->pad = 0;
}

}  // namespace

// The scan's grid: 4 slots a thread, at most two workgroups a CU's worth (they stride)
static uint32_t top_scan_grid(uint64_t cap) {
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (cap + 4 * kTopScanBlock - 1) / (4 * kTopScanBlock)), 512);
}

// After a scan left its matches in cand [cap] and its counters in T: the sum of
// row0 [w] into T->error_spans (nullptr, 0: none), then the select and the sort.
hipError_t launch_top_select(const unsigned long long *row0, uint32_t w, uint32_t k, uint64_t cap,
                             const ulonglong2 *cand, TopCtl *T, hipStream_t s) {
  hipLaunchKernelGGL(top_prepare_kernel, dim3(1), dim3(kTopBlock), 0, s, row0, w, k, T);
  // the select's workgroups stride the matches (at most cap); every digit's
  // launch is enqueued, the device decides which ones work -- none does when
  // the matches cannot outnumber what the sort holds (the prepare kernel sets
  // T->done), so those launches are left out
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (cap + 8 * kTopBlock - 1) / (8 * kTopBlock)), 1024);
  for (uint32_t digit = 0; digit < kTopDigits && cap > kTopSel; ++digit)
    hipLaunchKernelGGL(top_digit_kernel, dim3(grid), dim3(kTopBlock), 0, s, cand, T);
  hipLaunchKernelGGL(top_gather_kernel, dim3(grid), dim3(kTopBlock), 0, s, cand, T);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = hipFuncSetAttribute((const void *)&top_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)(kTopSel * sizeof(ulonglong2)));
      e != hipSuccess)
    return e;
  hipLaunchKernelGGL(top_sort_kernel, dim3(1), dim3(kTopSortBlock), kTopSel * sizeof(ulonglong2), s, T);
  return hipGetLastError();
}

hipError_t launch_top(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv, const unsigned long long *cells,
                      uint32_t d, uint32_t w, uint32_t shift, const uint64_t *seeds, uint32_t k,
                      unsigned long long min_count, ulonglong2 *cand, TopCtl *T, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(T, 0, offsetof(TopCtl, sel), s); e != hipSuccess) return e;
  const size_t cell_bytes = (size_t)d * w * 8;
  if (cell_bytes <= kTopCellsLds) {
    if (hipError_t e = hipFuncSetAttribute((const void *)&top_scan_kernel<1>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTopCellsLds);
        e != hipSuccess)
      return e;
    hipLaunchKernelGGL(top_scan_kernel<1>, dim3(top_scan_grid(cap)), dim3(kTopScanBlock), cell_bytes, s, gkeys, cap,
                       kinv, cells, d, w, shift, seeds, min_count, cand, T);
  } else {
    hipLaunchKernelGGL(top_scan_kernel<0>, dim3(top_scan_grid(cap)), dim3(kTopScanBlock), 0, s, gkeys, cap, kinv, cells,
                       d, w, shift, seeds, min_count, cand, T);
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  return launch_top_select(cells, w, k, cap, cand, T, s);
}

hipError_t launch_movers(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv, const unsigned long long *base,
                         const unsigned long long *cur, uint32_t d, uint32_t w, uint32_t shift, const uint64_t *seeds,
                         uint64_t nb, uint64_t nc, uint32_t fall, uint32_t k, unsigned long long min_score,
                         ulonglong2 *cand, TopCtl *T, MoversOut *O, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(T, 0, offsetof(TopCtl, sel), s); e != hipSuccess) return e;
  const size_t both_bytes = 2 * (size_t)d * w * 8;
  // the heavy hitters' grid; staged, both arrays are one workgroup a CU: at most 256 (they stride)
  const uint32_t grid = top_scan_grid(cap);
  if (both_bytes <= kMoversCellsLds) {
    if (hipError_t e = hipFuncSetAttribute((const void *)&movers_scan_kernel<1>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMoversCellsLds);
        e != hipSuccess)
      return e;
    hipLaunchKernelGGL(movers_scan_kernel<1>, dim3(std::min(grid, 256u)), dim3(kTopScanBlock), both_bytes, s, gkeys,
                       cap, kinv, base, cur, d, w, shift, seeds, nb, nc, fall, min_score, cand, T);
  } else {
    hipLaunchKernelGGL(movers_scan_kernel<0>, dim3(grid), dim3(kTopScanBlock), 0, s, gkeys, cap, kinv, base, cur, d, w,
                       shift, seeds, nb, nc, fall, min_score, cand, T);
  }
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = launch_top_select(cur, w, k, cap, cand, T, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(movers_rows_kernel, dim3((k + kTopBlock - 1) / kTopBlock), dim3(kTopBlock), 0, s, base, cur, d, w,
                     shift, seeds, T, O);
  return hipGetLastError();
}

// The tile and the stash of a width.  Up to 32 windows the whole block's
// suffix maxima fit kSeriesStashBytes at 64 columns (chunk = width).  Above,
// chunks: the stash holds chunk + ceil(width / chunk) entries of L columns,
// half the entries for each, so width <= chunk^2 -- 64 columns and chunks of
// 16 up to 256 windows, 32 and 32 up to 1,024, 16 and 64 up to 4,096 (the
// largest ring).
static void series_shape(uint32_t width, uint32_t *L, uint32_t *chunk) {
  *L = kSeriesLanes, *chunk = width;
  if ((uint64_t)width * kSeriesLanes * 16 <= kSeriesStashBytes) return;
  for (;; *L >>= 1) {
    *chunk = kSeriesStashBytes / 16 / *L / 2;
    if ((uint64_t)*chunk * *chunk >= width || *L == 1) return;
  }
}

hipError_t launch_series_hll(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p, uint64_t a,
                             uint32_t width, uint32_t n_out, uint32_t *hist, hipStream_t s) {
  uint32_t L, chunk;
  series_shape(width, &L, &chunk);
  const uint32_t log2tps = p - 4, C = (width + chunk - 1) / chunk;
  const uint64_t slot16 = (uint64_t)n_services << log2tps;
  const uint32_t per_block = width == 1 ? kSeriesChunk1 : width;  // outputs a workgroup takes
  const uint64_t tiles = (slot16 + L - 1) / L, blocks = (n_out + per_block - 1) / per_block;
  if (tiles * blocks >= (1ULL << 26)) return hipErrorInvalidConfiguration;  // (grid x block below 2^32)
  if (hipError_t e = hipMemsetAsync(hist, 0, (size_t)n_out * n_services * kRangeBins * 4, s); e != hipSuccess) return e;
  const uint32_t nsv = std::max(1u, L >> log2tps);
  const size_t lds = (width == 1 ? 0 : (size_t)(chunk + (C > 1 ? C : 0)) * L * 16) +
                     (size_t)(nsv == 1 ? kSeriesCopies * kSeriesCopyWords : nsv * kRangeBins) * 4;
  if (lds > 32768)  // (many services a tile)
    if (hipError_t e = hipFuncSetAttribute((const void *)&series_hll_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)lds);
        e != hipSuccess)
      return e;
  hipLaunchKernelGGL(series_hll_kernel, dim3((uint32_t)(tiles * blocks)), dim3(kSeriesLanes), lds, s,
                     reinterpret_cast<const uint4 *>(hll), slot16, n_windows - 1, a, width, n_out, log2tps, n_services,
                     L, chunk, (uint32_t)tiles, hist);
  return hipGetLastError();
}

hipError_t launch_series_query(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t a,
                               uint32_t width, uint32_t n_out, uint32_t d, uint32_t w, uint32_t shift,
                               const uint64_t *seeds, const uint64_t *keys, uint64_t n_keys, unsigned long long *out,
                               hipStream_t s) {
  if (n_keys == 0) return hipSuccess;
  const uint64_t key_blocks = (n_keys + 255) / 256;
  // chunks of the outputs: enough workgroups for a short key list (~2,048),
  // none shorter than a quarter of the seeding it pays for (width cells a
  // row), nor than 16 outputs
  const uint32_t most = std::max(1u, n_out / std::max(width / 4, 16u));
  const uint32_t chunks = (uint32_t)std::min<uint64_t>(most, std::max<uint64_t>(1, 2048 / key_blocks));
  const uint32_t per_chunk = (n_out + chunks - 1) / chunks;
  const dim3 grid((uint32_t)key_blocks, (n_out + per_chunk - 1) / per_chunk);
  hipLaunchKernelGGL(series_query_kernel, grid, dim3(256), 0, s, cms, slot_elems, n_windows - 1, a, width, n_out,
                     per_chunk, d, w, shift, seeds, keys, n_keys, out);
  return hipGetLastError();
}

hipError_t launch_series_row0(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t a,
                              uint32_t n_in, uint32_t w, unsigned long long *out, hipStream_t s) {
  hipLaunchKernelGGL(series_row0_kernel, dim3(n_in), dim3(256), 0, s, cms, slot_elems, n_windows - 1, a, w, out);
  return hipGetLastError();
}

hipError_t launch_range_merge(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p, uint64_t first,
                              uint32_t n_win, uint32_t *hist, uint8_t *out, hipStream_t s) {
  return launch_range_merge_sel(hll, n_windows, n_services, p, first, n_win, nullptr, n_services, hist, out, s);
}

hipError_t launch_range_merge_sel(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p,
                                  uint64_t first, uint32_t n_win, const uint32_t *svc_map, uint32_t n_sel,
                                  uint32_t *hist, uint8_t *out, hipStream_t s) {
  const uint32_t log2tps = p - 4, tiles = ((1u << log2tps) + 63) / 64;
  // workgroups a service: its tiles of 64 threads, fewer once the grid passes ~4,096 (they stride)
  const uint32_t wgs = std::max(1u, std::min(tiles, 4096u / std::min(n_sel, 4096u)));
  hipLaunchKernelGGL(range_merge_kernel, dim3(n_sel * wgs), dim3(kRangeBlock), 0, s,
                     reinterpret_cast<const uint4 *>(hll), (uint64_t)n_services << log2tps, n_windows - 1, first, n_win,
                     log2tps, wgs, svc_map, hist, reinterpret_cast<uint4 *>(out));
  return hipGetLastError();
}

hipError_t launch_range_fold(const unsigned long long *gkeys, unsigned long long *errcnt, uint64_t cap,
                             unsigned long long *cms, uint64_t slot_elems, uint32_t d, uint32_t w, uint32_t shift,
                             const uint64_t *seeds, uint64_t kinv, uint32_t dense, uint32_t n_windows, uint64_t first,
                             uint32_t n_win, hipStream_t s) {
  // a window's slots over its share of ~2,048 workgroups, at least 64 (they stride)
  const dim3 grid((uint32_t)std::min<uint64_t>((cap + 255) / 256, std::max(64u, 2048u / n_win)), n_win);
  hipLaunchKernelGGL(range_fold_kernel, grid, dim3(256), 0, s, gkeys, errcnt, cap, cms, slot_elems, d, w, shift, seeds,
                     kinv, dense, n_windows - 1, first);
  return hipGetLastError();
}

hipError_t launch_hll_hist(const uint8_t *merged, uint32_t n_services, uint32_t p, uint32_t *hist, hipStream_t s) {
  return launch_range_merge(merged, 1, n_services, p, 0, 1, hist, nullptr, s);
}

hipError_t launch_range_cells(const unsigned long long *cms, uint64_t slot_elems, uint32_t n_windows, uint64_t first,
                              uint32_t n_win, unsigned long long *out, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(out, 0, slot_elems * 8, s); e != hipSuccess) return e;
  const uint32_t per_chunk = (n_win + kCellChunks - 1) / kCellChunks;
  const dim3 grid((uint32_t)((slot_elems + 255) / 256), (n_win + per_chunk - 1) / per_chunk);
  hipLaunchKernelGGL(range_cells_kernel, grid, dim3(256), 0, s, cms, slot_elems, n_windows - 1, first, n_win, per_chunk,
                     out);
  return hipGetLastError();
}

hipError_t launch_range_query(const unsigned long long *cells, uint32_t d, uint32_t w, uint32_t shift,
                              const uint64_t *seeds, const uint64_t *keys, uint64_t n, unsigned long long *out,
                              hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(range_query_kernel, dim3((uint32_t)std::min<uint64_t>((n + 255) / 256, 2048)), dim3(256), 0, s,
                     cells, d, w, shift, seeds, keys, n, out);
  return hipGetLastError();
}

}  // namespace sa
