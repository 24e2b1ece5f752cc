// spanagg_overlap.hip -- the pair stage of sa_window_overlap /
// sa_group_window_overlap (gfx950; the merge stage is range_merge_kernel with a
// service map, spanagg_range.hip).
//
//   overlap_pairs_kernel  for every pair i < j of the n_sel merged register
//                         arrays: the value histogram of their register-wise
//                         maximum -- the HLL of the union of the two services'
//                         trace sets (every service's registers are filled
//                         from the same hash of the trace id).
//
// Unlike the kernels of spanagg_range.hip this one is not bound by a stream
// from HBM: n_sel x 2^p bytes (1 MiB at the defaults) are read n_sel - 1 times
// out of the caches, and the work is byte maxima and 2^p counts a pair.
//
// Blocking: the pair space is cut in tiles of 8 x 8 services (tile row ti <=
// tile column tj; a diagonal tile counts i < j only), the registers in chunks
// of columns (a column: 16 registers, one 16-byte word); one workgroup takes
// one tile and one chunk, its four waves count into the same 64 pair rows of 64
// bins in LDS, and it leaves one atomicAdd per non-zero bin.  Every count is
// an integer sum: the order of the atomics does not show.
//
// Counting ("Service overlap over the window ring", has
// the A/B): register values are geometrically distributed -- half of an array
// sits in two or three bins -- so where the lanes of a wave are 64 columns of
// ONE pair they meet on the same LDS words.  The kernel kept here makes the
// lanes the tile's 64 PAIRS instead: lane (a, b) owns row a * 8 + b, no two
// lanes ever share a word, and with rows of 65 words lanes that count the same
// value fall in different banks.  The laboratory build keeps the two
// column-wise forms to measure against.
#include <algorithm>

#include "sa_device.h"
#include "spanagg.h"

namespace sa {
namespace {

constexpr uint32_t kOvTile = 8;                      // services a tile side
constexpr uint32_t kOvPairs = kOvTile * kOvTile;     // pair rows a wave counts into
constexpr uint32_t kOvBins = SA_HLL_HIST_BINS;
constexpr uint32_t kOvRow = kOvBins + 1;             // words a pair row: equal values of neighbouring rows, other banks
constexpr uint32_t kOvBlock = 256;                   // four waves share the rows: LDS never bounds the waves a CU, one flush for four
constexpr uint32_t kOvWaves = kOvBlock / 64;
constexpr uint32_t kOvChunk = 64;                    // columns a workgroup takes, at least (lanes as columns: kOvBlock)
constexpr uint32_t kOvMaxChunks = 256;
constexpr uint32_t kOvInFlight = 4;                  // columns whose loads a lane issues before it counts them
static_assert(SA_OVERLAP_MAX_SERVICES % kOvTile == 0, "whole tiles at the largest selection");

__device__ __forceinline__ uint32_t ov_byte(const uint4 &m, uint32_t k) {
  const uint32_t w = k < 4 ? m.x : k < 8 ? m.y : k < 12 ? m.z : m.w;
  const uint32_t v = (w >> (8 * (k & 3))) & 0xFFu;
  return v < kOvBins ? v : kOvBins - 1;
}

// the 16 registers of m into the row at h, one LDS add each
__device__ __forceinline__ void ov_count(const uint4 &m, uint32_t *h) {
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) atomicAdd(&h[ov_byte(m, k)], 1u);
}

#ifdef SPANAGG_AB
// Column-wise forms (every lane of the wave runs this, `on` or not).  The
// values 0..3 hold 15/16 of a dense array: counted by ballot and popcount,
// lane 0 adds; the others one LDS add a lane.
__device__ __forceinline__ void ov_count_ballot(const uint4 &m, bool on, uint32_t *h) {
  const bool lane0 = (threadIdx.x & 63u) == 0;
#pragma unroll
  for (uint32_t k = 0; k < 16; ++k) {
    const uint32_t v = ov_byte(m, k);
    const uint64_t s0 = __ballot(on && v == 0), s1 = __ballot(on && v == 1), s2 = __ballot(on && v == 2),
                   s3 = __ballot(on && v == 3);
    if (lane0 && s0) atomicAdd(&h[0], (uint32_t)__popcll(s0));
    if (lane0 && s1) atomicAdd(&h[1], (uint32_t)__popcll(s1));
    if (lane0 && s2) atomicAdd(&h[2], (uint32_t)__popcll(s2));
    if (lane0 && s3) atomicAdd(&h[3], (uint32_t)__popcll(s3));
    if (on && v >= 4) atomicAdd(&h[v], 1u);
  }
}
#endif

// Variant 0 (the product's): lanes are pairs.  1: lanes are columns, a lane
// holds the 16 words of the tile's services in registers, one LDS add a
// register.  2: as 1 with ov_count_ballot.  (1 and 2: laboratory build only.)
// regs [n_sel][2^log2tps] words; pair_hist [n_sel (n_sel - 1) / 2][64] must be
// zero.  Grid: (tile pairs T (T + 1) / 2, chunks of `cols` columns).
template <int V>
__global__ __launch_bounds__(kOvBlock) void overlap_pairs_kernel(const uint4 *regs, uint32_t n_sel, uint32_t log2tps,
                                                                 uint32_t T, uint32_t cols, uint32_t *pair_hist) {
  __shared__ uint32_t h[kOvPairs * kOvRow];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, tps = 1u << log2tps;
  for (uint32_t i = threadIdx.x; i < kOvPairs * kOvRow; i += kOvBlock) h[i] = 0;
  uint32_t tp = blockIdx.x, ti = 0;  // tile row ti holds the T - ti tiles ti <= tj < T
  while (tp >= T - ti) tp -= T - ti, ++ti;
  const uint32_t i0 = ti * kOvTile, j0 = (ti + tp) * kOvTile;
  const uint32_t c0 = blockIdx.y * cols, c1 = min(tps, c0 + cols);
  __syncthreads();

  if constexpr (V == 0) {
    const uint32_t i = i0 + (lane >> 3), j = j0 + (lane & 7);
    const bool on = i < j && j < n_sel;  // (i < j < n_sel)
    const uint4 *A = regs + ((uint64_t)(on ? i : 0) << log2tps), *B = regs + ((uint64_t)(on ? j : 0) << log2tps);
    uint32_t *row = h + lane * kOvRow;
    for (uint32_t c = c0 + wave * kOvInFlight; c < c1; c += kOvWaves * kOvInFlight) {  // (the same trips for a wave's lanes)
      uint4 va[kOvInFlight], vb[kOvInFlight];
#pragma unroll
      for (uint32_t u = 0; u < kOvInFlight; ++u) {
        va[u] = vb[u] = uint4{0, 0, 0, 0};
        if (on && c + u < c1) va[u] = A[c + u], vb[u] = B[c + u];
      }
#pragma unroll
      for (uint32_t u = 0; u < kOvInFlight; ++u)
        if (on && c + u < c1) ov_count(max_u8x16(va[u], vb[u]), row);
    }
  }
#ifdef SPANAGG_AB
  else {
    for (uint32_t cb = c0; cb < c1; cb += kOvBlock) {  // (the same trips for every lane)
      const uint32_t c = cb + threadIdx.x;
      const bool on = c < c1;
      uint4 A[kOvTile], B[kOvTile];
#pragma unroll
      for (uint32_t a = 0; a < kOvTile; ++a) {
        A[a] = B[a] = uint4{0, 0, 0, 0};
        if (on && i0 + a < n_sel) A[a] = regs[((uint64_t)(i0 + a) << log2tps) + c];
        if (on && j0 + a < n_sel) B[a] = regs[((uint64_t)(j0 + a) << log2tps) + c];
      }
#pragma unroll
      for (uint32_t a = 0; a < kOvTile; ++a) {
#pragma unroll
        for (uint32_t b = 0; b < kOvTile; ++b) {
          if (i0 + a < j0 + b && j0 + b < n_sel) {  // (uniform)
            const uint4 m = max_u8x16(A[a], B[b]);
            uint32_t *row = h + (a * kOvTile + b) * kOvRow;
            if constexpr (V == 2) {
              ov_count_ballot(m, on, row);
            } else {
              if (on) ov_count(m, row);
            }
          }
        }
      }
    }
  }
#endif

  __syncthreads();
  for (uint32_t x = threadIdx.x; x < kOvPairs * kOvBins; x += kOvBlock) {
    const uint32_t pr = x / kOvBins, bin = x % kOvBins;
    const uint32_t i = i0 + pr / kOvTile, j = j0 + pr % kOvTile;
    if (i >= j || j >= n_sel) continue;
    const uint32_t n = h[pr * kOvRow + bin];
    const uint32_t pair = i * n_sel - i * (i + 1) / 2 + (j - i - 1);  // < n_sel (n_sel - 1) / 2
    if (n) atomicAdd(pair_hist + (uint64_t)pair * kOvBins + bin, n);
  }
}

}  // namespace

hipError_t launch_overlap_pairs(const uint8_t *regs, uint32_t n_sel, uint32_t p, uint32_t *pair_hist, uint32_t variant,
                                hipStream_t s) {
  if (n_sel < 2) return hipSuccess;
  if (n_sel > SA_OVERLAP_MAX_SERVICES || p < 4 || p > 18) return hipErrorInvalidValue;
  const uint32_t log2tps = p - 4, tps = 1u << log2tps;
  const uint32_t T = (n_sel + kOvTile - 1) / kOvTile;
  const uint32_t chunk = variant == 0 ? kOvChunk : kOvBlock;  // (lanes as columns: a column a thread)
  const uint32_t chunks = std::min(kOvMaxChunks, (tps + chunk - 1) / chunk);
  const uint32_t cols = (tps + chunks - 1) / chunks;
  const dim3 grid(T * (T + 1) / 2, (tps + cols - 1) / cols);
  const uint4 *r = reinterpret_cast<const uint4 *>(regs);
#ifdef SPANAGG_AB
  if (variant == 1)
    hipLaunchKernelGGL(overlap_pairs_kernel<1>, grid, dim3(kOvBlock), 0, s, r, n_sel, log2tps, T, cols, pair_hist);
  else if (variant == 2)
    hipLaunchKernelGGL(overlap_pairs_kernel<2>, grid, dim3(kOvBlock), 0, s, r, n_sel, log2tps, T, cols, pair_hist);
  else
#endif
  {
    if (variant != 0) return hipErrorInvalidValue;  // (the product library holds one kernel)
    hipLaunchKernelGGL(overlap_pairs_kernel<0>, grid, dim3(kOvBlock), 0, s, r, n_sel, log2tps, T, cols, pair_hist);
  }
  return hipGetLastError();
}

}  // namespace sa
