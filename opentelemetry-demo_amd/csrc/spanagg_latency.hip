// spanagg_latency.hip -- latency histograms over the window ring (gfx950), for
// SA_OPT_WINDOW_LATENCY engines and sa_window_latency / sa_group_window_latency
// (engine_ingest.cpp, engine_read.cpp, spanagg_group.cpp).
//
//   lat_ingest_kernel  one streaming pass over start_ns, end_ns and meta (20 B
//                      a span) beside the launch's ingest kernel: every span
//                      that updates an HLL register -- a valid service, an end
//                      inside the ring (window_slot, the same launch
//                      parameters) -- adds one to ring[slot][service][bin].
//                      Up to kLatLdsServices services a workgroup counts a few
//                      consecutive ring slots in LDS, pass by pass over its
//                      range, and adds the non-zero cells after each pass.
//   lat_sums_kernel    the sliding sums of one service's rows over the
//                      windows: the entering window added, the leaving one
//                      subtracted, one wave a (service, chunk of outputs).
//   lat_scan_kernel    a summed row's count and quantile bins: lane-local
//                      prefix, wave scan, ballot.
//
// The two query stages are apart because a group adds its members' sums
// between them.  Every cell is an integer sum, so the order of the atomics
// does not show: two calls, and one engine against a group, give the same bits.
#include <algorithm>
#include <cstddef>

#include "sa_device.h"
#include "sa_latency.h"
#include "spanagg.h"

namespace sa {
namespace {

static_assert(kLatBins == SA_LAT_BINS, "one bin count");
constexpr uint32_t kLatBlock = 1024;
constexpr uint32_t kLatNoSlot = 0xFFFFFFFFu;
constexpr uint32_t kLatQueryBlock = 256;  // four waves: a row (scan) or a (service, chunk) (sums) each
constexpr uint32_t kLatSumWaves = 2048;   // the sums stage splits the outputs into chunks up to this many waves
constexpr uint32_t kLatMaxPasses = 8;     // the ingest kernel's passes over a range whose spans are out of time order

// The spans a workgroup has in LDS during one pass: the k_slots ring slots from
// home + rel0 on.
struct LatPass {
  uint32_t home, rel0, k_slots;
  bool last;  // the spans of later slots go to the ring now (no pass follows)
};

// One span into its cell: LDS when its slot is one of the pass's, the ring
// otherwise; true when a later pass has to take it.  The ring index stays
// below n_windows * n_services * 256 (window_slot < n_windows, svc <
// n_services, latency_bin < 256), the LDS index below k_slots * n_services * 256.
template <bool LDS>
__device__ __forceinline__ bool lat_count(const IngestParams &P, unsigned long long *ring, uint32_t *cells,
                                          const LatPass &L, uint64_t start, uint64_t end, uint32_t meta) {
  const uint32_t svc = meta & 0xFFFFu;
  const uint32_t ws = window_slot(P, end);
  if (svc >= P.n_services || ws == kLatNoSlot) return false;
  const uint32_t cell = (svc << 8) | latency_bin(end > start ? end - start : 0);
  if (LDS && L.home != kLatNoSlot) {
    const uint32_t rel = (ws - L.home) & P.win_mask;  // the slot's place behind the home slot
    if (rel - L.rel0 < L.k_slots) {
      atomicAdd(cells + (rel - L.rel0) * (P.n_services << 8) + cell, 1u);
      return false;
    }
    if (rel < L.rel0) return false;  // (an earlier pass counted it)
    if (!L.last) return true;
  }
  atomicAdd(ring + (((uint64_t)ws * P.n_services) << 8) + cell, 1ULL);
  return false;
}

// Workgroup b counts spans [b * chunk, (b + 1) * chunk) (chunk a multiple of 4:
// the u64 columns stay 16-byte aligned, meta 8-byte).  LDS: cells [k_slots]
// [n_services][256] u32 of dynamic LDS hold k_slots consecutive ring slots from
// the home slot on -- the slot of the first in-ring span of the range, found
// kLatBlock spans at a time (none: nothing to count).  A time-ordered
// batch takes one pass: its spans lie in the home slot or the next.  Spans of
// later slots wait for a later pass over the range, which holds the next
// k_slots slots, up to kLatMaxPasses; the last pass sends what is left
// straight to the ring.  After each pass the non-zero cells are added to the
// ring, a row of consecutive bins a wave.  A cell counts at most chunk < 2^32
// spans.
template <bool LDS>
__global__ __launch_bounds__(kLatBlock) void lat_ingest_kernel(IngestParams P, unsigned long long *ring, uint64_t chunk,
                                                               uint32_t k_slots) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint32_t s_first, s_home;
  uint32_t *cells = reinterpret_cast<uint32_t *>(smem);
  const uint32_t tid = threadIdx.x, ncell = P.n_services << 8;
  uint64_t lo = (uint64_t)blockIdx.x * chunk;
  if (lo > P.n) lo = P.n;
  const uint64_t hi = lo + chunk < P.n ? lo + chunk : P.n;
  LatPass L{kLatNoSlot, 0, k_slots, true};
  if (LDS) {
    for (uint32_t i = tid; i < k_slots * (ncell / 4); i += kLatBlock)
      reinterpret_cast<uint4 *>(cells)[i] = uint4{0, 0, 0, 0};
    if (tid == 0) s_first = kLatNoSlot, s_home = kLatNoSlot;
    __syncthreads();
    for (uint64_t at = lo; at < hi; at += kLatBlock) {  // (the same trips for every thread)
      const uint32_t ws = at + tid < hi ? window_slot(P, P.end[at + tid]) : kLatNoSlot;
      if (!__syncthreads_or(ws != kLatNoSlot ? 1 : 0)) continue;
      if (ws != kLatNoSlot) atomicMin(&s_first, tid);
      __syncthreads();
      if (ws != kLatNoSlot && s_first == tid) s_home = ws;
      break;
    }
    __syncthreads();
    L.home = s_home;
    if (L.home == kLatNoSlot) return;  // (uniform: no span of the range is in the ring)
  }
  const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(P.start + lo);
  const ulonglong2 *e2 = reinterpret_cast<const ulonglong2 *>(P.end + lo);
  const uint2 *m2 = reinterpret_cast<const uint2 *>(P.meta + lo);
  const uint64_t npair = (hi - lo) >> 1;
  for (uint32_t pass = 0;; ++pass) {
    L.rel0 = pass * k_slots;
    L.last = !LDS || L.home == kLatNoSlot || pass + 1 == kLatMaxPasses || L.rel0 + k_slots > P.win_mask;
    bool left = false;
    // two spans a lane and load, two loads in flight
    uint64_t i = tid;
    for (; i + kLatBlock < npair; i += 2 * kLatBlock) {
      const ulonglong2 sa = s2[i], ea = e2[i], sb = s2[i + kLatBlock], eb = e2[i + kLatBlock];
      const uint2 ma = m2[i], mb = m2[i + kLatBlock];
      left |= lat_count<LDS>(P, ring, cells, L, sa.x, ea.x, ma.x);
      left |= lat_count<LDS>(P, ring, cells, L, sa.y, ea.y, ma.y);
      left |= lat_count<LDS>(P, ring, cells, L, sb.x, eb.x, mb.x);
      left |= lat_count<LDS>(P, ring, cells, L, sb.y, eb.y, mb.y);
    }
    for (; i < npair; i += kLatBlock) {
      const ulonglong2 sa = s2[i], ea = e2[i];
      const uint2 ma = m2[i];
      left |= lat_count<LDS>(P, ring, cells, L, sa.x, ea.x, ma.x);
      left |= lat_count<LDS>(P, ring, cells, L, sa.y, ea.y, ma.y);
    }
    if (((hi - lo) & 1) && tid == 0)  // (the batch's last span: n odd)
      left |= lat_count<LDS>(P, ring, cells, L, P.start[hi - 1], P.end[hi - 1], P.meta[hi - 1]);
    if (!LDS || L.home == kLatNoSlot) break;  // (uniform: nothing is in LDS)
    __syncthreads();
    for (uint32_t j = 0; j < k_slots; ++j) {
      // (a slot past the ring's last holds nothing: every rel is below n_windows)
      unsigned long long *row = ring + (((uint64_t)((L.home + L.rel0 + j) & P.win_mask) * P.n_services) << 8);
      for (uint32_t c = tid; c < ncell; c += kLatBlock)
        if (const uint32_t v = cells[j * ncell + c]) {
          atomicAdd(row + c, (unsigned long long)v);
          cells[j * ncell + c] = 0;  // (for the next pass; the barrier below orders it before that pass's adds)
        }
    }
    if (!__syncthreads_or(left ? 1 : 0) || L.last) break;
  }
}

struct U64x4 {
  unsigned long long v[4];
};
__device__ __forceinline__ U64x4 lat_row(const unsigned long long *p) {
  const ulonglong2 a = reinterpret_cast<const ulonglong2 *>(p)[0], b = reinterpret_cast<const ulonglong2 *>(p)[1];
  return U64x4{{a.x, a.y, b.x, b.y}};
}

// Wave w serves selected service w / n_chunks and outputs [c * chunk, (c + 1) *
// chunk) of n_out, c = w % n_chunks; output o covers windows a + o .. a + o +
// width - 1 of the ring [win_mask + 1][n_services][256] (a + n_out + width - 2
// resident: the caller checked).  Lane l holds bins 4l .. 4l + 3: a row is one
// coalesced 2 KiB read.  sums [n_out][n_sel][256].  A window is read twice,
// and once more where a chunk starts.
__global__ __launch_bounds__(kLatQueryBlock) void lat_sums_kernel(const unsigned long long *__restrict__ ring,
                                                                  uint32_t n_services, uint32_t win_mask,
                                                                  const uint32_t *__restrict__ sel, uint32_t n_sel,
                                                                  uint64_t a, uint32_t width, uint32_t n_out,
                                                                  uint32_t chunk, uint32_t n_chunks,
                                                                  unsigned long long *__restrict__ sums) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t w = (uint64_t)blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (w >= (uint64_t)n_sel * n_chunks) return;  // (wave-uniform)
  const uint32_t s = (uint32_t)(w / n_chunks), o0 = (uint32_t)(w % n_chunks) * chunk;
  const uint32_t o1 = min(n_out, o0 + chunk);
  const uint64_t at = ((uint64_t)sel[s] << 8) + lane * 4;
  auto row = [&](uint32_t k) { return lat_row(ring + ((((a + k) & win_mask) * n_services) << 8) + at); };
  U64x4 acc{{0, 0, 0, 0}};
  for (uint32_t k = o0; k + 1 < o0 + width; ++k) {
    const U64x4 r = row(k);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.v[j] += r.v[j];
  }
#pragma unroll 4
  for (uint32_t o = o0; o < o1; ++o) {
    const U64x4 in = row(o + width - 1), out = row(o);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.v[j] += in.v[j];
    ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(sums + (((uint64_t)o * n_sel + s) << 8) + lane * 4);
    dst[0] = ulonglong2{acc.v[0], acc.v[1]};
    dst[1] = ulonglong2{acc.v[2], acc.v[3]};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc.v[j] -= out.v[j];
  }
}

struct LatQuantiles {
  uint32_t n, ppm[SA_LAT_MAX_Q];
};

// One wave a row of sums [n_rows][256]: count[row] = the row's total, q_bin[row]
// [i] = the smallest bin whose cumulative count reaches r = max(1, ceil(count *
// ppm[i] / 10^6)) (count * ppm < 2^64 while count < 2^44), 0 for an empty row.
__global__ __launch_bounds__(kLatQueryBlock) void lat_scan_kernel(const unsigned long long *__restrict__ sums,
                                                                  uint64_t n_rows, LatQuantiles Q,
                                                                  unsigned long long *__restrict__ count,
                                                                  uint8_t *__restrict__ q_bin) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;  // (wave-uniform)
  const U64x4 v = lat_row(sums + (r << 8) + lane * 4);
  const unsigned long long p0 = v.v[0], p1 = p0 + v.v[1], p2 = p1 + v.v[2], p3 = p2 + v.v[3];
  unsigned long long incl = p3;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  const unsigned long long total = __shfl(incl, 63), excl = incl - p3;
  if (lane == 0) count[r] = total;
  for (uint32_t i = 0; i < Q.n; ++i) {
    unsigned long long rank = (total * Q.ppm[i] + 999999ULL) / 1000000ULL;
    if (rank == 0) rank = 1;
    const unsigned long long reached = __ballot(incl >= rank);
    const uint32_t j = excl + p0 >= rank ? 0u : excl + p1 >= rank ? 1u : excl + p2 >= rank ? 2u : 3u;
    uint32_t bin = 0;
    if (reached) {  // (total >= rank >= 1: some lane reaches it)
      const uint32_t first = (uint32_t)__ffsll((long long)reached) - 1u;
      bin = first * 4 + (uint32_t)__shfl((int)j, (int)first);
    }
    if (lane == 0) q_bin[r * Q.n + i] = (uint8_t)bin;
  }
}

}  // namespace

hipError_t prepare_lat_ingest(size_t lds_bytes) {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(lat_ingest_kernel<true>),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
}

hipError_t launch_lat_ingest(const IngestParams &P, unsigned long long *ring, uint32_t grid, uint64_t chunk,
                             uint32_t k_slots, hipStream_t s) {
  if (k_slots)
    hipLaunchKernelGGL(lat_ingest_kernel<true>, dim3(grid), dim3(kLatBlock), (size_t)k_slots * P.n_services * 1024, s, P,
                       ring, chunk, k_slots);
  else
    hipLaunchKernelGGL(lat_ingest_kernel<false>, dim3(grid), dim3(kLatBlock), 0, s, P, ring, chunk, 0u);
  return hipGetLastError();
}

hipError_t launch_lat_sums(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows, const uint32_t *sel,
                           uint32_t n_sel, uint64_t a, uint32_t width, uint32_t n_out, unsigned long long *sums,
                           hipStream_t s) {
  // chunks of outputs, each at least max(width, 4) long (a chunk re-reads width
  // - 1 windows), until about kLatSumWaves waves are in flight
  const uint32_t longest = std::max(1u, n_out / std::max(width, 4u));
  const uint32_t n_chunks0 = std::max(1u, std::min(longest, kLatSumWaves / std::max(1u, n_sel)));
  const uint32_t chunk = (n_out + n_chunks0 - 1) / n_chunks0, n_chunks = (n_out + chunk - 1) / chunk;
  const uint64_t waves = (uint64_t)n_sel * n_chunks, per = kLatQueryBlock / 64;
  hipLaunchKernelGGL(lat_sums_kernel, dim3((uint32_t)((waves + per - 1) / per)), dim3(kLatQueryBlock), 0, s, ring,
                     n_services, n_windows - 1, sel, n_sel, a, width, n_out, chunk, n_chunks, sums);
  return hipGetLastError();
}

hipError_t launch_lat_scan(const unsigned long long *sums, uint64_t n_rows, const uint32_t *q_ppm, uint32_t n_q,
                           unsigned long long *count, uint8_t *q_bin, hipStream_t s) {
  LatQuantiles Q{};
  Q.n = std::min<uint32_t>(n_q, SA_LAT_MAX_Q);
  for (uint32_t i = 0; i < Q.n; ++i) Q.ppm[i] = q_ppm[i];
  const uint64_t per = kLatQueryBlock / 64;
  hipLaunchKernelGGL(lat_scan_kernel, dim3((uint32_t)((n_rows + per - 1) / per)), dim3(kLatQueryBlock), 0, s, sums,
                     n_rows, Q, count, q_bin);
  return hipGetLastError();
}

}  // namespace sa
