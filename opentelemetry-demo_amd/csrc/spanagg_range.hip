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
//   range_cells_kernel   count-min cells summed over the windows (u64).
//   range_query_kernel   point queries on the summed cells, one thread a key.
//
// Every result is an integer maximum or an integer sum, so the order of the
// atomics does not show: two calls, and one engine against a group, give the
// same bits.
#include <algorithm>

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

// max of four u8 lanes, each below 128 (an HLL register is at most 65 - p):
// (a | 0x80) - b keeps bit 7 exactly where a >= b and borrows from no neighbour
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b) {
  const uint32_t ge = (((a | 0x80808080u) - b) >> 7) & 0x01010101u;
  const uint32_t m = ge * 0xFFu;
  return (a & m) | (b & ~m);
}
__device__ __forceinline__ uint4 max_u8x16(uint4 a, uint4 b) {
  return uint4{max_u8x4(a.x, b.x), max_u8x4(a.y, b.y), max_u8x4(a.z, b.z), max_u8x4(a.w, b.w)};
}

// Workgroup b serves service b / wgs and strides the service's tiles of 64
// threads; a thread owns 16 consecutive registers (tps = 2^log2tps threads a
// service, 2^p = 16 tps).  The workgroup's four waves each walk a quarter of
// the windows for the same tile -- a 512 MB ring of 32 services is 512 tiles,
// two waves a CU if a tile were one wave's -- and their partial maxima meet
// in LDS; wave 0 stores and counts.  regs: [win_mask + 1][n_services][2^p].
// hist (nullptr: none) [n_services][64] must be zero; out (nullptr: none)
// [n_services][2^p].
__global__ __launch_bounds__(kRangeBlock) void range_merge_kernel(const uint4 *regs, uint64_t slot16, uint32_t win_mask,
                                                                  uint64_t first, uint32_t n_win, uint32_t log2tps,
                                                                  uint32_t wgs, uint32_t *hist, uint4 *out) {
  __shared__ uint32_t h[kRangeBins];  // wave 0's histogram
  __shared__ uint4 part[kRangeWaves - 1][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kRangeBins) h[threadIdx.x] = 0;  // (ordered before the first count by the loop's barrier)
  const uint32_t svc = blockIdx.x / wgs, wg = blockIdx.x % wgs, tps = 1u << log2tps;
  const uint32_t per = (n_win + kRangeWaves - 1) / kRangeWaves;
  const uint32_t k0 = min(n_win, wave * per), k1 = min(n_win, k0 + per);
  for (uint32_t t = wg; t < (tps + 63) / 64; t += wgs) {  // (the same trips for every thread)
    const uint32_t c = t * 64 + lane;
    const uint64_t at = ((uint64_t)svc << log2tps) + c;
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
      if (out) out[at] = acc;
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

}  // namespace

hipError_t launch_range_merge(const uint8_t *hll, uint32_t n_windows, uint32_t n_services, uint32_t p, uint64_t first,
                              uint32_t n_win, uint32_t *hist, uint8_t *out, hipStream_t s) {
  const uint32_t log2tps = p - 4, tiles = ((1u << log2tps) + 63) / 64;
  // workgroups a service: its tiles of 64 threads, fewer once the grid passes ~4,096 (they stride)
  const uint32_t wgs = std::max(1u, std::min(tiles, 4096u / std::min(n_services, 4096u)));
  hipLaunchKernelGGL(range_merge_kernel, dim3(n_services * wgs), dim3(kRangeBlock), 0, s,
                     reinterpret_cast<const uint4 *>(hll), (uint64_t)n_services << log2tps, n_windows - 1, first, n_win,
                     log2tps, wgs, hist, reinterpret_cast<uint4 *>(out));
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
