// spanagg_error_onset.hip -- when each series began to fail (gfx950), for
// sa_window_error_onset / sa_group_window_error_onset (engine_window.cpp,
// spanagg_group.cpp): every split of a range of windows tried for every key
// resident in the key table, the best split's score ranked by the heavy
// hitters' select and sort (spanagg_range.hip).
//
//   error_onset_scan_kernel  the key table against the summed cells (a key's
//                            S_r and E: ineligible keys leave here) and then
//                            against the windows' own cells: one walk with the
//                            d running prefixes gives every split's D and the
//                            best one; (D, key) of every match (sa_device.h's
//                            table_scan, the best D as its score).
//   error_onset_rows_kernel  the selected keys walk again: the split, B and A.
//
// The windows are read as (base, stride, first, mask): window j of the range
// is at base + ((first + j) & mask) * stride -- the engine's ring (mask =
// n_windows - 1) or a group's merged, unwrapped [n][d * w] array (first 0, a
// mask of all ones).  A lane owns a candidate; the laboratory build also holds
// the scan with a wave a candidate ("Error onset over the
// window ring").  Sums and minima of integers only: two calls,
// and one engine against a group, give the same bits.
#include <algorithm>
#include <cstddef>

#include "sa_device.h"
#include "spanagg.h"

namespace sa {
namespace {

constexpr uint32_t kEoScanBlock = 256;  // four waves: a slot a thread, the walk's registers decide the occupancy
constexpr uint32_t kEoBlock = 256;
// windows whose d gathers a lane issues before it adds them to its prefixes
// (the gathers are independent, only the adds chain)
#ifndef SA_ERROR_ONSET_IN_FLIGHT
#define SA_ERROR_ONSET_IN_FLIGHT 4
#endif
constexpr uint32_t kEoInFlight = SA_ERROR_ONSET_IN_FLIGHT;

struct EoWindows {
  const unsigned long long *cells;
  uint64_t stride, first, mask;
  uint32_t n;
};

struct EoSplit {
  unsigned long long t, before, after;
  long long score;
};

// The key's cell of each row within a window's [d][w], its sums S over the
// range from sum [d][w], and their minimum E.
__device__ __forceinline__ unsigned long long eo_columns(const unsigned long long *sum, uint32_t d, uint32_t w,
                                                         uint32_t shift, const uint64_t (&sd)[8], uint64_t key,
                                                         uint64_t (&at)[8], unsigned long long (&S)[8]) {
  unsigned long long E = ~0ULL;
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) {  // (cms_d <= 8)
    at[r] = 0, S[r] = 0;
    if (r < d) {
      at[r] = (uint64_t)r * w + (splitmix64(key ^ sd[r]) >> shift);  // col < w: shift = 64 - log2 w, w >= 2
      S[r] = sum[at[r]];
      E = S[r] < E ? S[r] : E;
    }
  }
  return E;
}

// Every split t = 1 .. n - 1 of the range in one pass: after window t - 1
// joined the prefixes P, B = min P_r, A = min (S_r - P_r), D = A * t - B * (n -
// t) (two's complement: the signed difference; negated when fall).  The
// largest D, the latest among equal ones; t = 0 when there is no split.
__device__ __forceinline__ EoSplit eo_walk(const EoWindows &W, uint32_t d, const uint64_t (&at)[8],
                                           const unsigned long long (&S)[8], uint32_t fall) {
  EoSplit best{0, 0, 0, (long long)(1ULL << 63)};
  unsigned long long P[8];
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) P[r] = 0;
  const uint32_t n = W.n, splits = n - 1;  // (n >= 1)
  const auto step = [&](uint32_t t, const unsigned long long (&x)[8]) {
    unsigned long long B = ~0ULL, A = ~0ULL;
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) {
      if (r < d) {
        P[r] += x[r];
        const unsigned long long a = S[r] - P[r];
        B = P[r] < B ? P[r] : B;
        A = a < A ? a : A;
      }
    }
    unsigned long long D = A * t - B * (n - t);
    if (fall) D = 0ULL - D;
    if ((long long)D >= best.score) best = EoSplit{t, B, A, (long long)D};
  };
  uint32_t j = 0;
  for (; j + kEoInFlight <= splits; j += kEoInFlight) {
    unsigned long long x[kEoInFlight][8];
#pragma unroll
    for (uint32_t u = 0; u < kEoInFlight; ++u) {
      const unsigned long long *slot = W.cells + ((W.first + j + u) & W.mask) * W.stride;
#pragma unroll
      for (uint32_t r = 0; r < 8; ++r) x[u][r] = r < d ? slot[at[r]] : 0;
    }
#pragma unroll
    for (uint32_t u = 0; u < kEoInFlight; ++u) step(j + u + 1, x[u]);
  }
  for (; j < splits; ++j) {
    const unsigned long long *slot = W.cells + ((W.first + j) & W.mask) * W.stride;
    unsigned long long x[8];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) x[r] = r < d ? slot[at[r]] : 0;
    step(j + 1, x);
  }
  return best;
}

// table_scan with a key's best D as its score.  sum [d][w], the windows'
// cells summed, is staged in LDS (LDS = 1: d * w * 8 <= kTopCellsLds dynamic
// bytes) or read through global memory; the windows themselves are read
// through global memory.  Keys with E >= min_count (>= 1) are eligible and
// counted into O->n_eligible; of those, the keys with a best D >= min_score
// (>= 1, so the score orders as an unsigned number) match.
template <int LDS>
__global__ __launch_bounds__(kEoScanBlock) void error_onset_scan_kernel(const unsigned long long *gkeys, uint64_t cap,
                                                                        uint64_t kinv, const unsigned long long *sum,
                                                                        EoWindows W, uint32_t d, uint32_t w,
                                                                        uint32_t shift, const uint64_t *seeds,
                                                                        uint32_t fall, unsigned long long min_count,
                                                                        unsigned long long min_score, ulonglong2 *cand,
                                                                        TopCtl *T, ErrOnsetOut *O) {
  extern __shared__ unsigned long long eo_cells[];
  const unsigned long long *c = sum;
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < d * w; i += kEoScanBlock) eo_cells[i] = sum[i];
    __syncthreads();
    c = eo_cells;
  }
  uint64_t sd[8];  // (cms_d <= 8)
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
  uint32_t eligible = 0;
  table_scan<kEoScanBlock>(gkeys, cap, kinv, cand, T, [&](uint64_t key, unsigned long long &score) {
    uint64_t at[8];
    unsigned long long S[8];
    if (eo_columns(c, d, w, shift, sd, key, at, S) < min_count) return false;
    ++eligible;
    const EoSplit best = eo_walk(W, d, at, S, fall);
    score = (unsigned long long)best.score;
    return best.score >= 1 && score >= min_score;
  });
  eligible = wave_sum(eligible);
  if ((threadIdx.x & 63u) == 0 && eligible) atomicAdd(&O->n_eligible, (unsigned long long)eligible);
}

#ifdef SPANAGG_AB
// Laboratory (variant 1): a wave owns a candidate.  Every lane takes a table
// slot and its key's columns as the product's scan does; then the wave serves
// its eligible lanes one at a time: the candidate's columns and sums are
// broadcast, lane l takes window j0 + l of 64, a wave scan of the d rows gives
// every lane its prefixes (plus the carry of the steps before), every lane
// scores its own split, and the wave takes the largest D, the latest among
// equal ones.  Same matches, counters and candidate frame as the product's.
template <int LDS>
__global__ __launch_bounds__(kEoScanBlock) void error_onset_scan_wave_kernel(
    const unsigned long long *gkeys, uint64_t cap, uint64_t kinv, const unsigned long long *sum, EoWindows W, uint32_t d,
    uint32_t w, uint32_t shift, const uint64_t *seeds, uint32_t fall, unsigned long long min_count,
    unsigned long long min_score, ulonglong2 *cand, TopCtl *T, ErrOnsetOut *O) {
  extern __shared__ unsigned long long eo_cells[];
  const unsigned long long *c = sum;
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < d * w; i += kEoScanBlock) eo_cells[i] = sum[i];
    __syncthreads();
    c = eo_cells;
  }
  uint64_t sd[8];
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
  const uint32_t lane = threadIdx.x & 63u, n = W.n, splits = n - 1;
  uint32_t resident = 0, eligible = 0;
  unsigned long long largest = 0;
  for (uint64_t s0 = blockIdx.x * (uint64_t)kEoScanBlock + (threadIdx.x & ~63u); s0 < cap;
       s0 += (uint64_t)gridDim.x * kEoScanBlock) {  // (the same trips for a wave's lanes)
    const uint64_t key = s0 + lane < cap ? gkeys[s0 + lane] * kinv : 0;
    uint64_t at[8];
    unsigned long long S[8];
#pragma unroll
    for (uint32_t r = 0; r < 8; ++r) at[r] = 0, S[r] = 0;
    bool elig = false;
    if (key) {
      ++resident;
      elig = eo_columns(c, d, w, shift, sd, key, at, S) >= min_count;
      if (elig) ++eligible;
    }
    unsigned long long score = 0;
    bool match = false;
    for (uint64_t todo = __ballot(elig); todo; todo &= todo - 1) {
      const int src = __ffsll((unsigned long long)todo) - 1;
      uint64_t cat[8];
      unsigned long long cS[8], carry[8];
#pragma unroll
      for (uint32_t r = 0; r < 8; ++r) cat[r] = __shfl(at[r], src), cS[r] = __shfl(S[r], src), carry[r] = 0;
      long long bD = (long long)(1ULL << 63);
      uint32_t bt = 0;
      for (uint32_t j0 = 0; j0 < splits; j0 += 64) {
        const uint32_t j = j0 + lane;
        const bool on = j < splits;
        const unsigned long long *slot = W.cells + ((W.first + j) & W.mask) * W.stride;
        unsigned long long B = ~0ULL, A = ~0ULL;
#pragma unroll
        for (uint32_t r = 0; r < 8; ++r) {
          if (r < d) {  // (uniform)
            unsigned long long x = on ? slot[cat[r]] : 0;
#pragma unroll
            for (uint32_t dd = 1; dd < 64; dd <<= 1) {
              const unsigned long long up = __shfl_up(x, dd);
              if (lane >= dd) x += up;
            }
            x += carry[r];
            carry[r] = __shfl(x, 63);
            const unsigned long long a = cS[r] - x;
            B = x < B ? x : B;
            A = a < A ? a : A;
          }
        }
        if (on) {
          const uint32_t t = j + 1;
          unsigned long long D = A * t - B * (n - t);
          if (fall) D = 0ULL - D;
          if ((long long)D >= bD) bD = (long long)D, bt = t;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const long long oD = __shfl_xor(bD, o);
        const uint32_t ot = __shfl_xor(bt, o);
        if (oD > bD || (oD == bD && ot > bt)) bD = oD, bt = ot;
      }
      if ((int)lane == src) score = (unsigned long long)bD, match = bD >= 1 && score >= min_score;
    }
    if (match) {
      largest = score > largest ? score : largest;
      const unsigned long long pos = wave_ticket(&T->n_matched, __ballot(true));
      if (pos < cap) cand[pos] = ulonglong2{score, key};
    }
  }
  resident = wave_sum(resident), eligible = wave_sum(eligible);
  largest = wave_max_u64(largest);
  if (lane == 0) {
    if (resident) atomicAdd(&T->n_resident, (unsigned long long)resident);
    if (largest) atomicMax(&T->max_est, largest);
    if (eligible) atomicAdd(&O->n_eligible, (unsigned long long)eligible);
  }
}
#endif

// a scan kernel, and the largest `variant` the build holds
using EoScan = void (*)(const unsigned long long *, uint64_t, uint64_t, const unsigned long long *, EoWindows, uint32_t,
                        uint32_t, uint32_t, const uint64_t *, uint32_t, unsigned long long, unsigned long long,
                        ulonglong2 *, TopCtl *, ErrOnsetOut *);
#ifdef SPANAGG_AB
constexpr uint32_t kEoVariants = 1;
#else
constexpr uint32_t kEoVariants = 0;
#endif

// After the sort: O->row[i] = the best split of row i of T->sel, i < T->want
// (<= kTopSel), from the same arrays the scan read.
__global__ __launch_bounds__(kEoBlock) void error_onset_rows_kernel(const unsigned long long *sum, EoWindows W,
                                                                    uint32_t d, uint32_t w, uint32_t shift,
                                                                    const uint64_t *seeds, uint32_t fall,
                                                                    const TopCtl *T, ErrOnsetOut *O) {
  const uint32_t i = blockIdx.x * kEoBlock + threadIdx.x;
  if (i >= T->want || i >= kTopSel) return;
  uint64_t sd[8], at[8];
  unsigned long long S[8];
#pragma unroll
  for (uint32_t r = 0; r < 8; ++r) sd[r] = r < d ? seeds[r] : 0;
  eo_columns(sum, d, w, shift, sd, T->sel[i].y, at, S);
  const EoSplit best = eo_walk(W, d, at, S, fall);
  O->row[i] = ErrOnsetRow{best.t, best.before, best.after};
}

}  // namespace

hipError_t launch_error_onset(const unsigned long long *gkeys, uint64_t cap, uint64_t kinv,
                              const unsigned long long *sum, const unsigned long long *win_cells, uint64_t win_stride,
                              uint64_t first, uint64_t mask, uint32_t n_win, uint32_t d, uint32_t w, uint32_t shift,
                              const uint64_t *seeds, uint32_t fall, uint32_t k, unsigned long long min_count,
                              unsigned long long min_score, ulonglong2 *cand, TopCtl *T, ErrOnsetOut *O, uint32_t variant,
                              hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(T, 0, offsetof(TopCtl, sel), s); e != hipSuccess) return e;
  if (hipError_t e = hipMemsetAsync(O, 0, offsetof(ErrOnsetOut, row), s); e != hipSuccess) return e;
  const EoWindows W{win_cells, win_stride, first, mask, n_win};
  // a slot a thread, at most 2,048 workgroups (they stride)
  const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (cap + kEoScanBlock - 1) / kEoScanBlock), 2048);
  const size_t cell_bytes = (size_t)d * w * 8;
  const bool staged = cell_bytes <= kTopCellsLds;
  EoScan scan = staged ? error_onset_scan_kernel<1> : error_onset_scan_kernel<0>;
#ifdef SPANAGG_AB
  if (variant == 1) scan = staged ? error_onset_scan_wave_kernel<1> : error_onset_scan_wave_kernel<0>;
#endif
  if (variant > kEoVariants) return hipErrorInvalidValue;  // (the product library holds one kernel)
  if (staged)
    if (hipError_t e = hipFuncSetAttribute((const void *)scan, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)kTopCellsLds);
        e != hipSuccess)
      return e;
  hipLaunchKernelGGL(scan, dim3(grid), dim3(kEoScanBlock), staged ? cell_bytes : 0, s, gkeys, cap, kinv, sum, W, d, w,
                     shift, seeds, fall, min_count, min_score, cand, T, O);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = launch_top_select(sum, w, k, cap, cand, T, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(error_onset_rows_kernel, dim3((k + kEoBlock - 1) / kEoBlock), dim3(kEoBlock), 0, s, sum, W, d, w,
                     shift, seeds, fall, T, O);
  return hipGetLastError();
}

}  // namespace sa
