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
//   lat_range_sums_kernel, lat_score_kernel, lat_mov_rows_kernel
//                      sa_window_latency_movers: two ranges' rows summed per
//                      service (one range for the onset's pooled threshold; a
//                      long range split over waves), every service
//                      scored by the shift of its ranking quantile's bin --
//                      the select and the sort are the heavy hitters' -- and
//                      the selected services' counts and bins.
//   slo_pairs_kernel, slo_slide_kernel
//                      sa_window_slo: every covered (window, service) row cut
//                      to a (total, slow) pair at the service's threshold bin
//                      -- the ring read once whatever the widths -- then
//                      prefix sums along the windows, every width's sums as
//                      the difference of two prefixes, and the burn rule.
//   onset_thr_kernel, onset_scan_kernel, onset_rows_kernel
//                      sa_window_latency_onset: every service's pooled quantile
//                      bin from its rows summed over the range (the range
//                      sums kernel, one range), its (total, slow) pairs (the
//                      SLO's pairs kernel), then per service the split of the
//                      range with the largest D = S_a N_b - S_b N_a in 128
//                      bits, the change of the slow share as the score -- the
//                      select and the sort are the heavy hitters' -- and the
//                      selected services' records.
//
// The two service-ranking scans (lat_score_kernel, onset_scan_kernel) share
// sa_device.h's candidate frame -- a workgroup's matches in LDS, one place
// range in cand and one set of atomics a workgroup (RankList) -- and one grid
// rule; the SLO's and the onset's prefix over (total, slow) pairs is one
// pair_scan_step; every wave read of a summed row is lat_sum_row.
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
static_assert(sizeof(LatMovRow::q_bin) == 2 * SA_LAT_MAX_Q, "a row's bins hold the most quantiles");
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

// A wave's view of one row of 256 bins, lane l holding bins 4l .. 4l + 3: p[j] =
// the lane's own bins 0..j summed, incl / excl = the wave's prefix over the
// lanes' sums with and without this lane's, total = the row's count (every lane).
struct LatRowScan {
  unsigned long long p[4], incl, excl, total;
};
__device__ __forceinline__ LatRowScan lat_row_scan(const U64x4 &v, uint32_t lane) {
  LatRowScan R;
  R.p[0] = v.v[0], R.p[1] = R.p[0] + v.v[1], R.p[2] = R.p[1] + v.v[2], R.p[3] = R.p[2] + v.v[3];
  unsigned long long incl = R.p[3];
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(incl, d);
    if (lane >= d) incl += t;
  }
  R.incl = incl, R.excl = incl - R.p[3], R.total = __shfl(incl, 63);
  return R;
}
// The quantile rule (every lane of the wave calls it, every lane gets the
// answer): the smallest bin whose cumulative count reaches r = max(1,
// ceil(total * ppm / 10^6)) (total * ppm < 2^64 while total < 2^44), 0 for an
// empty row.
__device__ __forceinline__ uint32_t lat_quantile_bin(const LatRowScan &R, uint32_t ppm) {
  unsigned long long rank = (R.total * ppm + 999999ULL) / 1000000ULL;
  if (rank == 0) rank = 1;
  const unsigned long long reached = __ballot(R.incl >= rank);
  const uint32_t j = R.excl + R.p[0] >= rank ? 0u : R.excl + R.p[1] >= rank ? 1u : R.excl + R.p[2] >= rank ? 2u : 3u;
  uint32_t bin = 0;
  if (reached) {  // (total >= rank >= 1: some lane reaches it)
    const uint32_t first = (uint32_t)__ffsll((long long)reached) - 1u;
    bin = first * 4 + (uint32_t)__shfl((int)j, (int)first);
  }
  return bin;
}
// The wave's view of row `row` of sums [..][256]
__device__ __forceinline__ LatRowScan lat_sum_row(const unsigned long long *sums, uint64_t row, uint32_t lane) {
  return lat_row_scan(lat_row(sums + (row << 8) + lane * 4), lane);
}

// One wave a row of sums [n_rows][256]: count[row] = the row's total, q_bin[row]
// [i] = lat_quantile_bin of ppm[i].
__global__ __launch_bounds__(kLatQueryBlock) void lat_scan_kernel(const unsigned long long *__restrict__ sums,
                                                                  uint64_t n_rows, LatQuantiles Q,
                                                                  unsigned long long *__restrict__ count,
                                                                  uint8_t *__restrict__ q_bin) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (r >= n_rows) return;  // (wave-uniform)
  const LatRowScan R = lat_sum_row(sums, r, lane);
  if (lane == 0) count[r] = R.total;
  for (uint32_t i = 0; i < Q.n; ++i) {
    const uint32_t bin = lat_quantile_bin(R, Q.ppm[i]);
    if (lane == 0) q_bin[r * Q.n + i] = (uint8_t)bin;
  }
}

// ---- latency movers (sa_window_latency_movers): both ranges' rows summed per
// service, every service scored by the shift of its ranking quantile's bin,
// the select and the sort the heavy hitters' (spanagg_range.hip), then the
// selected services' rows ----
constexpr uint32_t kLatPairBlock = 256;   // four waves: stripes of one unit, or one-stripe units
constexpr uint32_t kLatPairWaves = 4096;  // the sums split units into stripes up to about this many waves
constexpr uint32_t kLatStripeRows = 8;    // ... and no finer than this many windows a stripe
// the service-ranking scans' workgroups (RankList, sa_device.h), while a wave
// then has no more than kLatScoreIters services (65,536 services: exactly both)
constexpr uint32_t kLatScoreGrid = 512;

// Range sums over n_ranges in {1, 2}.  Unit u = r * n_services + s is service
// s over range r < n_ranges (sa_window_latency_movers: 0 the baseline, 1 the
// current one; sa_window_latency_onset sums one range, first_c and len_c unread):
// windows first[r] .. first[r] + len[r] - 1.  A unit is `stripes`
// waves (1, 2 or a multiple of 4, so the waves of a workgroup that share a
// unit are `grp` = min(stripes, 4) neighbours); stripe t sums the t-th run of
// ceil(len / stripes) consecutive windows of the unit (interleaved stripes
// took 8 % longer on a 1,024-window ring) -- lane l bins 4l .. 4l + 3, a row
// one coalesced 2 KiB read, four rows in flight -- and the grp waves add up
// through LDS.
// Up to 4 stripes the first wave stores the unit's row of sums [n_ranges]
// [n_services][256]; above, the workgroups of a unit add theirs to the row (zeroed by the
// launcher) -- integer adds, so neither the split nor the order shows.  The
// ring index stays below (win_mask + 1) * n_services * 256: s < n_services, and
// k < len[r] <= win_mask + 1.
__global__ __launch_bounds__(kLatPairBlock) void lat_range_sums_kernel(const unsigned long long *__restrict__ ring,
                                                                      uint32_t n_services, uint32_t win_mask,
                                                                      uint64_t first_b, uint32_t len_b, uint64_t first_c,
                                                                      uint32_t len_c, uint32_t n_ranges,
                                                                      uint32_t stripes, uint32_t grp,
                                                                      unsigned long long *__restrict__ sums) {
  __shared__ unsigned long long part[kLatPairBlock / 64][SA_LAT_BINS];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t gw = (uint64_t)blockIdx.x * (kLatPairBlock / 64) + wv;
  const uint64_t u = gw / stripes;
  const uint32_t t = (uint32_t)(gw % stripes);
  const bool live = u < (uint64_t)n_ranges * n_services;  // (wave-uniform; a dead wave still meets the barrier)
  U64x4 acc{{0, 0, 0, 0}};
  if (live) {
    const uint32_t r = u >= n_services ? 1u : 0u, s = (uint32_t)(u - (uint64_t)r * n_services);
    const uint64_t first = r ? first_c : first_b;
    const uint32_t len = r ? len_c : len_b;
    const uint64_t at = ((uint64_t)s << 8) + lane * 4;
    const uint32_t per = (len + stripes - 1) / stripes, k0 = min(len, t * per), k1 = min(len, k0 + per);
#pragma unroll 4
    for (uint32_t k = k0; k < k1; ++k) {
      const U64x4 v = lat_row(ring + ((((first + k) & win_mask) * n_services) << 8) + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.v[j] += v.v[j];
    }
  }
  if (grp > 1) {  // (a launch parameter: every thread takes the same side)
    const uint32_t lead = wv & ~(grp - 1);
    if (wv != lead) {
      ulonglong2 *dst = reinterpret_cast<ulonglong2 *>(&part[wv][lane * 4]);
      dst[0] = ulonglong2{acc.v[0], acc.v[1]};
      dst[1] = ulonglong2{acc.v[2], acc.v[3]};
    }
    __syncthreads();
    if (wv != lead) return;
    for (uint32_t o = 1; o < grp; ++o) {
      const U64x4 v = lat_row(&part[lead + o][lane * 4]);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc.v[j] += v.v[j];
    }
  }
  if (!live) return;
  unsigned long long *dst = sums + (u << 8) + lane * 4;
  if (stripes <= 4) {
    reinterpret_cast<ulonglong2 *>(dst)[0] = ulonglong2{acc.v[0], acc.v[1]};
    reinterpret_cast<ulonglong2 *>(dst)[1] = ulonglong2{acc.v[2], acc.v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (acc.v[j]) atomicAdd(dst + j, acc.v[j]);
  }
}

struct LatMovParams {
  unsigned long long min_count;  // >= 1
  uint32_t min_shift;            // >= 1 (above 255: nothing matches)
  uint32_t fall, ppm0;
};

// One wave a service s of sums [2][n_services][256] at a time, the waves of the
// grid striding the services: both counts (into counts [2][n_services]) and
// both ranking-quantile bins; eligible when both counts reach min_count, shift
// = cur's bin - base's (negated when fall), a match when eligible with shift
// >= min_shift.  A match leaves as (score, s), score = (shift << 48) |
// min(count_cur, 2^48 - 1): ordered as the heavy hitters' pairs -- score
// descending, then id ascending -- that is (shift, count_cur) descending, then
// id ascending.  The matches and the tallies go through RankList (sa_device.h):
// cand [n_services], T->n_resident the eligible, and O->spans_base and
// O->spans_cur the sums of the two counts.
__global__ __launch_bounds__(kLatScoreBlock) void lat_score_kernel(const unsigned long long *__restrict__ sums,
                                                                   uint32_t n_services, LatMovParams M,
                                                                   unsigned long long *__restrict__ counts,
                                                                   ulonglong2 *__restrict__ cand, TopCtl *T,
                                                                   LatMovOut *O) {
  __shared__ RankList<2> list;
  constexpr uint32_t kWaves = RankList<2>::kWaves;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  list.init();
  unsigned long long largest = 0, spans[2] = {0, 0};  // (the wave's own, the same in every lane: base, cur)
  uint32_t ne = 0;
  for (uint32_t s = blockIdx.x * kWaves + wv; s < n_services; s += gridDim.x * kWaves) {  // (wave-uniform)
    const LatRowScan B = lat_sum_row(sums, s, lane), C = lat_sum_row(sums, (uint64_t)n_services + s, lane);
    const uint32_t bb = lat_quantile_bin(B, M.ppm0), bc = lat_quantile_bin(C, M.ppm0);
    spans[0] += B.total, spans[1] += C.total;
    const bool elig = B.total >= M.min_count && C.total >= M.min_count;
    ne += elig ? 1u : 0u;
    const int32_t shift = M.fall ? (int32_t)bb - (int32_t)bc : (int32_t)bc - (int32_t)bb;
    if (lane == 0) counts[s] = B.total, counts[(uint64_t)n_services + s] = C.total;
    if (elig && shift >= 1 && (uint32_t)shift >= M.min_shift) {
      const unsigned long long top = (1ULL << 48) - 1;
      const unsigned long long score = ((unsigned long long)(uint32_t)shift << 48) | (C.total < top ? C.total : top);
      largest = score > largest ? score : largest;
      if (lane == 0) list.push(score, s);
    }
  }
  unsigned long long *const span_out[2] = {&O->spans_base, &O->spans_cur};
  list.publish(largest, ne, spans, n_services, cand, T, span_out);
}

// After the sort, one wave a row i < T->want of T->sel: the service's two
// counts and, for both of its summed rows, every quantile's bin -- O->row[i]
// (the rule lat_scan_kernel applies, on the same sums).
__global__ __launch_bounds__(kLatQueryBlock) void lat_mov_rows_kernel(const unsigned long long *__restrict__ sums,
                                                                      uint32_t n_services, LatQuantiles Q,
                                                                      const TopCtl *T, LatMovOut *O) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (i >= T->want || i >= kTopSel) return;  // (wave-uniform)
  const uint64_t s = T->sel[i].y;
  if (s >= n_services) return;  // (a candidate is a service id: never taken)
  for (uint32_t r = 0; r < 2; ++r) {
    const LatRowScan R = lat_sum_row(sums, (uint64_t)r * n_services + s, lane);
    if (lane == 0) O->row[i].count[r] = R.total;
    for (uint32_t q = 0; q < SA_LAT_MAX_Q; ++q) {  // (the unasked ones 0: the row is copied whole)
      const uint32_t bin = q < Q.n ? lat_quantile_bin(R, Q.ppm[q]) : 0u;
      if (lane == 0) O->row[i].q_bin[r][q] = (uint8_t)bin;
    }
  }
}

// ---- latency SLO burn (sa_window_slo): every covered row cut to a (total,
// slow) pair at its service's threshold bin, then -- after a group has added
// its members' pairs -- prefix sums along the windows, every width's
// difference of two prefixes, and the burn rule ----
constexpr uint32_t kSloSlideBlock = 64;  // one wave: a service's scan carries from chunk to chunk

struct SloRule {
  uint32_t n, max_width;  // the widths asked for, the longest
  uint32_t width[SA_SLO_MAX_WIDTHS], limit_ppm[SA_SLO_MAX_WIDTHS];
  unsigned long long min_count;  // >= 1
};

// Wave r serves covered window k = r / n_sel (window a + k of the ring
// [win_mask + 1][n_services][256]; a + n_cov - 1 resident: the caller checked)
// and selected service i = r % n_sel, so neighbouring waves read neighbouring
// rows of one window (sel == nullptr: service i itself, n_sel <= n_services --
// sa_window_latency_onset's every service).  Lane l holds bins 4l .. 4l + 3 -- the row is one
// coalesced 2 KiB read -- and counts as slow those above thr_bin[i]; lane 0
// writes pairs[i][k] = {total, slow}, pairs [n_sel][n_cov]: a service's
// windows lie side by side for the scan.  The ring index stays below (win_mask
// + 1) * n_services * 256 (sel[i] < n_services: the host checked; 4l + 3 <
// 256), the pairs index below n_sel * n_cov (r < n_cov * n_sel).
__global__ __launch_bounds__(kLatQueryBlock) void slo_pairs_kernel(const unsigned long long *__restrict__ ring,
                                                                   uint32_t n_services, uint32_t win_mask,
                                                                   const uint32_t *__restrict__ sel,
                                                                   const uint8_t *__restrict__ thr_bin, uint32_t n_sel,
                                                                   uint64_t a, uint32_t n_cov,
                                                                   ulonglong2 *__restrict__ pairs) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t r = (uint64_t)blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (r >= (uint64_t)n_cov * n_sel) return;  // (wave-uniform)
  const uint32_t k = (uint32_t)(r / n_sel), i = (uint32_t)(r % n_sel);
  const U64x4 v = lat_row(ring + (((((a + k) & win_mask) * n_services) + (sel ? sel[i] : i)) << 8) + lane * 4);
  const uint32_t tb = thr_bin[i];
  unsigned long long total = 0, slow = 0;
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    total += v.v[j];
    slow += lane * 4 + j > tb ? v.v[j] : 0ULL;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    total += __shfl_xor(total, o);
    slow += __shfl_xor(slow, o);
  }
  if (lane == 0) pairs[(uint64_t)i * n_cov + k] = ulonglong2{total, slow};
}

// One wave (a workgroup of its own) a selected service i.  The scan: 64 windows
// of pairs [n_sel][n_cov] a step -- one coalesced 1 KiB read -- a wave scan
// and the carry of the steps before give P[i][k + 1] = pairs[i][0..k] summed,
// P [n_sel][n_cov + 1] with P[i][0] = 0.  Then, once the barrier has made the
// wave's own stores visible to all its lanes, 64 outputs a step: output o ends
// at covered window R.max_width - 1 + o, so width w covers P[i][e] - P[i][e -
// R.width[w]] with e = R.max_width + o -- e <= R.max_width + n_out - 1 = n_cov,
// and e - width >= 0 as width <= max_width -- written to total and slow
// [n_out][R.n][n_sel]; bit w of burning [n_out][n_sel] is the burn rule
// (strict, both products in u64), and alert[i] counts the outputs whose R.n
// bits are all set.  Every sum is an integer: neither the split into steps nor
// a group's order of adding shows.
__global__ __launch_bounds__(kSloSlideBlock) void slo_slide_kernel(const ulonglong2 *__restrict__ pairs, uint32_t n_sel,
                                                                   uint32_t n_cov, uint32_t n_out, SloRule R,
                                                                   ulonglong2 *P_all,
                                                                   unsigned long long *__restrict__ total,
                                                                   unsigned long long *__restrict__ slow,
                                                                   uint8_t *__restrict__ burning,
                                                                   uint32_t *__restrict__ alert) {
  const uint32_t lane = threadIdx.x, i = blockIdx.x;
  const ulonglong2 *p = pairs + (uint64_t)i * n_cov;
  ulonglong2 *P = P_all + (uint64_t)i * (n_cov + 1ull);
  if (lane == 0) P[0] = ulonglong2{0, 0};
  ulonglong2 carry{0, 0};
  for (uint32_t k0 = 0; k0 < n_cov; k0 += 64) {  // (the same trips for every lane)
    const uint32_t k = k0 + lane;
    const ulonglong2 ts = pair_scan_step(p, k, n_cov, lane, carry);
    if (k < n_cov) P[k + 1] = ts;
  }
  __threadfence_block();
  __syncthreads();
  const uint32_t all = (1u << R.n) - 1u;
  uint32_t alerts = 0;
  for (uint32_t o0 = 0; o0 < n_out; o0 += 64) {
    const uint32_t o = o0 + lane;
    uint32_t bits = 0;
    if (o < n_out) {
      const uint32_t e = R.max_width + o;
      const ulonglong2 hi = P[e];
      for (uint32_t w = 0; w < R.n; ++w) {
        const ulonglong2 lo = P[e - R.width[w]];
        const unsigned long long t = hi.x - lo.x, s = hi.y - lo.y;
        const uint64_t at = ((uint64_t)o * R.n + w) * n_sel + i;
        total[at] = t, slow[at] = s;
        if (t >= R.min_count && s * 1000000ULL > (unsigned long long)R.limit_ppm[w] * t) bits |= 1u << w;
      }
      burning[(uint64_t)o * n_sel + i] = (uint8_t)bits;
    }
    alerts += (uint32_t)__popcll(__ballot(o < n_out && bits == all));
  }
  if (lane == 0) alert[i] = alerts;
}

// ---- latency onset (sa_window_latency_onset): every service's threshold bin
// -- given, or the pooled quantile's of its rows summed over the range -- its
// (total, slow) pairs by slo_pairs_kernel, then -- after a group has added its
// members' pairs -- per service the split of the range with the largest D, the
// candidates' select and sort (the heavy hitters'), and the selected rows ----

// One wave a row of sums [n_services][256] (the range's rows summed,
// lat_range_sums_kernel over one range): thr_bin[s] = lat_quantile_bin of ppm,
// sa_window_latency's rule, 0 for a service without spans.  s < n_services.
__global__ __launch_bounds__(kLatQueryBlock) void onset_thr_kernel(const unsigned long long *__restrict__ sums,
                                                                   uint32_t n_services, uint32_t ppm,
                                                                   uint8_t *__restrict__ thr_bin) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t s = blockIdx.x * (kLatQueryBlock / 64) + (threadIdx.x >> 6);
  if (s >= n_services) return;  // (wave-uniform)
  const uint32_t bin = lat_quantile_bin(lat_sum_row(sums, s, lane), ppm);
  if (lane == 0) thr_bin[s] = (uint8_t)bin;
}

struct OnsetParams {
  unsigned long long min_count;  // >= 1
  uint32_t min_delta;            // >= 1 (above 10^6: nothing matches)
  uint32_t fall;
};
constexpr unsigned long long kOnsetCountTop = (1ULL << 44) - 1;  // a candidate's count, clamped for the order

// One wave a service s of pairs [n_sel][n_cov] at a time, the waves of the grid
// striding the services (lat_score_kernel's geometry).  First the range's sums
// N and S, a lane every 64th window.  Then the prefix scan, 64 windows a step
// with a carry (pair_scan_step, as slo_slide_kernel's): lane l of step k0 holds N_b and S_b of
// split t = k0 + l + 1 (before = windows 0 .. t - 1), a split while t <=
// n_cov - 1; eligible with N_b and N_a = N - N_b both >= min_count; D = S_a N_b
// - S_b N_a (negated when fall) as a signed 128-bit integer -- the products
// reach 2^88 while N < 2^44.  A lane keeps the best of its own splits (>=: its
// later split wins a tie), and after the steps a wave argmax takes (D, t), the
// larger t among equal D: t differs from lane to lane, so every lane ends with
// the same split.  t == 0: no eligible split.  Then delta_ppm = floor(S_a 10^6 /
// N_a) - floor(S_b 10^6 / N_b) in u64 (negated when fall), a match when D > 0
// and delta_ppm >= min_delta; it leaves as (score, s), score = (delta_ppm <<
// 44) | min(N, 2^44 - 1) -- delta_ppm <= 10^6 < 2^20 -- ordered as the heavy
// hitters' pairs.  rec[s] takes the split and its four sums (zeros without an
// eligible split).  The matches and the tallies go through RankList as
// lat_score_kernel's: cand [n_sel], T->n_resident the eligible, O->spans.  The
// pairs index stays below n_sel * n_cov (s < n_sel, k < n_cov), rec's below n_sel.
__global__ __launch_bounds__(kLatScoreBlock) void onset_scan_kernel(const ulonglong2 *__restrict__ pairs,
                                                                    uint32_t n_sel, uint32_t n_cov, OnsetParams M,
                                                                    OnsetRow *__restrict__ rec,
                                                                    ulonglong2 *__restrict__ cand, TopCtl *T,
                                                                    OnsetOut *O) {
  __shared__ RankList<1> list;
  constexpr uint32_t kWaves = RankList<1>::kWaves;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  list.init();
  unsigned long long largest = 0, spans[1] = {0};  // (the wave's own, the same in every lane)
  uint32_t ne = 0;
  for (uint32_t s = blockIdx.x * kWaves + wv; s < n_sel; s += gridDim.x * kWaves) {  // (wave-uniform)
    const ulonglong2 *p = pairs + (uint64_t)s * n_cov;
    unsigned long long N = 0, S = 0;
    for (uint32_t k = lane; k < n_cov; k += 64) {
      const ulonglong2 v = p[k];
      N += v.x, S += v.y;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) N += __shfl_xor(N, o), S += __shfl_xor(S, o);
    __int128 best_d = 0;
    unsigned long long best_nb = 0, best_sb = 0;
    ulonglong2 carry{0, 0};
    uint32_t best_t = 0;
    for (uint32_t k0 = 0; k0 + 1 < n_cov; k0 += 64) {  // (the same trips for every lane; the last window ends no split)
      const uint32_t k = k0 + lane;
      const ulonglong2 before = pair_scan_step(p, k, n_cov, lane, carry);
      const unsigned long long nb = before.x, sb = before.y, na = N - nb, sa = S - sb;
      if (k + 1 < n_cov && nb >= M.min_count && na >= M.min_count) {
        __int128 d = (__int128)sa * (__int128)nb - (__int128)sb * (__int128)na;
        if (M.fall) d = -d;
        if (best_t == 0 || d >= best_d) best_d = d, best_t = k + 1, best_nb = nb, best_sb = sb;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t ot = __shfl_xor(best_t, o);
      const unsigned long long lo = __shfl_xor((unsigned long long)best_d, o);
      const long long hi = __shfl_xor((long long)(best_d >> 64), o);
      const unsigned long long onb = __shfl_xor(best_nb, o), osb = __shfl_xor(best_sb, o);
      const __int128 od = (__int128)(((unsigned __int128)(unsigned long long)hi << 64) | lo);
      if (ot && (best_t == 0 || od > best_d || (od == best_d && ot > best_t)))
        best_d = od, best_t = ot, best_nb = onb, best_sb = osb;
    }
    spans[0] += N;
    const bool elig = best_t != 0;
    ne += elig ? 1u : 0u;
    const unsigned long long na = elig ? N - best_nb : 0, sa = elig ? S - best_sb : 0;
    long long delta = 0;
    if (elig) {  // (N_b, N_a >= min_count >= 1; S 10^6 < 2^64 while S < 2^44)
      delta = (long long)(sa * 1000000ULL / na) - (long long)(best_sb * 1000000ULL / best_nb);
      if (M.fall) delta = -delta;
    }
    if (lane == 0) rec[s] = OnsetRow{best_t, best_nb, best_sb, na, sa, 0};
    if (elig && best_d > 0 && delta >= 1 && delta >= (long long)M.min_delta) {
      const unsigned long long score = ((unsigned long long)delta << 44) | (N < kOnsetCountTop ? N : kOnsetCountTop);
      largest = score > largest ? score : largest;
      if (lane == 0) list.push(score, s);
    }
  }
  unsigned long long *const span_out[1] = {&O->spans};
  list.publish(largest, ne, spans, n_sel, cand, T, span_out);
}

// After the sort, one thread a row i < T->want of T->sel: the service's record
// with its threshold bin (thr_bin == nullptr: 0) -- O->row[i].  i < kTopSel.
__global__ __launch_bounds__(kLatQueryBlock) void onset_rows_kernel(const OnsetRow *__restrict__ rec,
                                                                    const uint8_t *__restrict__ thr_bin,
                                                                    uint32_t n_sel, const TopCtl *T, OnsetOut *O) {
  const uint32_t i = blockIdx.x * kLatQueryBlock + threadIdx.x;
  if (i >= T->want || i >= kTopSel) return;
  const uint64_t s = T->sel[i].y;
  if (s >= n_sel) return;  // (a candidate is a service id: never taken)
  OnsetRow r = rec[s];
  r.thr_bin = thr_bin ? thr_bin[s] : 0;
  O->row[i] = r;
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

// The stripes a (range, service) unit's windows are split into for the longest
// range `len` (1, 2 or a multiple of 4): a power of two, no more than fill
// about kLatPairWaves waves over two ranges' units, none finer than kLatStripeRows windows.
static uint32_t lat_range_stripes(uint32_t n_services, uint32_t len) {
  uint32_t stripes = 1;
  while (2 * stripes * 2ull * n_services <= kLatPairWaves && stripes * kLatStripeRows < len) stripes *= 2;
  return stripes;
}

// The service-ranking scans' grid: a service a wave up to kLatScoreGrid
// workgroups, then several -- no more than a workgroup's list holds
static uint32_t lat_score_grid(uint32_t n) {
  const uint32_t per = kLatScoreBlock / 64;
  return std::max(std::min((n + per - 1) / per, kLatScoreGrid), (n + kLatScoreList - 1) / kLatScoreList);
}

hipError_t launch_lat_range_sums(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows,
                                 const uint64_t *range, uint32_t n_ranges, unsigned long long *sums, hipStream_t s) {
  const uint64_t first_b = range[0], first_c = n_ranges > 1 ? range[2] : 0;
  const uint32_t len_b = (uint32_t)(range[1] - range[0] + 1), len_c = n_ranges > 1 ? (uint32_t)(range[3] - range[2] + 1) : 0;
  const uint32_t stripes = lat_range_stripes(n_services, std::max(len_b, len_c));
  const uint64_t units = (uint64_t)n_ranges * n_services, waves = units * stripes, per = kLatPairBlock / 64;
  if (stripes > 4)  // (the workgroups of a unit add to its row)
    if (hipError_t e = hipMemsetAsync(sums, 0, units * SA_LAT_BINS * 8, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(lat_range_sums_kernel, dim3((uint32_t)((waves + per - 1) / per)), dim3(kLatPairBlock), 0, s, ring,
                     n_services, n_windows - 1, first_b, len_b, first_c, len_c, n_ranges, stripes, std::min(stripes, 4u),
                     sums);
  return hipGetLastError();
}

hipError_t launch_lat_movers(const unsigned long long *sums, uint32_t n_services, uint32_t k,
                             unsigned long long min_count, uint32_t min_shift, uint32_t fall, const uint32_t *q_ppm,
                             uint32_t n_q, unsigned long long *counts, ulonglong2 *cand, TopCtl *T, LatMovOut *O,
                             hipStream_t s) {
  LatQuantiles Q{};
  Q.n = std::min<uint32_t>(n_q, SA_LAT_MAX_Q);
  for (uint32_t i = 0; i < Q.n; ++i) Q.ppm[i] = q_ppm[i];
  if (hipError_t e = hipMemsetAsync(T, 0, offsetof(TopCtl, sel), s); e != hipSuccess) return e;
  if (hipError_t e = hipMemsetAsync(O, 0, offsetof(LatMovOut, row), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(lat_score_kernel, dim3(lat_score_grid(n_services)), dim3(kLatScoreBlock), 0, s, sums, n_services,
                     LatMovParams{min_count, min_shift, fall, Q.ppm[0]}, counts, cand, T, O);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  // (no row to sum: the score kernel took both ranges' spans)
  if (hipError_t e = launch_top_select(nullptr, 0, k, n_services, cand, T, s); e != hipSuccess) return e;
  const uint32_t rows_per = kLatQueryBlock / 64;
  hipLaunchKernelGGL(lat_mov_rows_kernel, dim3((k + rows_per - 1) / rows_per), dim3(kLatQueryBlock), 0, s, sums,
                     n_services, Q, T, O);
  return hipGetLastError();
}

hipError_t launch_slo_pairs(const unsigned long long *ring, uint32_t n_services, uint32_t n_windows, const uint32_t *sel,
                            const uint8_t *thr_bin, uint32_t n_sel, uint64_t a, uint32_t n_cov,
                            unsigned long long *pairs, hipStream_t s) {
  const uint64_t waves = (uint64_t)n_cov * n_sel, per = kLatQueryBlock / 64;
  hipLaunchKernelGGL(slo_pairs_kernel, dim3((uint32_t)((waves + per - 1) / per)), dim3(kLatQueryBlock), 0, s, ring,
                     n_services, n_windows - 1, sel, thr_bin, n_sel, a, n_cov, reinterpret_cast<ulonglong2 *>(pairs));
  return hipGetLastError();
}

hipError_t launch_slo_slide(const unsigned long long *pairs, uint32_t n_sel, uint32_t n_out, const uint32_t *widths,
                            const uint32_t *limit_ppm, uint32_t n_widths, unsigned long long min_count,
                            unsigned long long *prefix, unsigned long long *total, unsigned long long *slow,
                            uint8_t *burning, uint32_t *alert, hipStream_t s) {
  SloRule R{};
  R.n = std::min<uint32_t>(n_widths, SA_SLO_MAX_WIDTHS);
  for (uint32_t w = 0; w < R.n; ++w) {
    R.width[w] = widths[w], R.limit_ppm[w] = limit_ppm[w];
    R.max_width = std::max(R.max_width, widths[w]);
  }
  R.min_count = min_count;
  hipLaunchKernelGGL(slo_slide_kernel, dim3(n_sel), dim3(kSloSlideBlock), 0, s,
                     reinterpret_cast<const ulonglong2 *>(pairs), n_sel, n_out + R.max_width - 1, n_out, R,
                     reinterpret_cast<ulonglong2 *>(prefix), total, slow, burning, alert);
  return hipGetLastError();
}

hipError_t launch_onset_thr(const unsigned long long *sums, uint32_t n_services, uint32_t q_ppm, uint8_t *thr_bin,
                            hipStream_t s) {
  const uint32_t per = kLatQueryBlock / 64;
  hipLaunchKernelGGL(onset_thr_kernel, dim3((n_services + per - 1) / per), dim3(kLatQueryBlock), 0, s, sums, n_services,
                     q_ppm, thr_bin);
  return hipGetLastError();
}

hipError_t launch_onset(const unsigned long long *pairs, uint32_t n_sel, uint32_t n_cov, uint32_t k,
                        unsigned long long min_count, uint32_t min_delta, uint32_t fall, const uint8_t *thr_bin,
                        OnsetRow *rec, ulonglong2 *cand, TopCtl *T, OnsetOut *O, hipStream_t s) {
  if (hipError_t e = hipMemsetAsync(T, 0, offsetof(TopCtl, sel), s); e != hipSuccess) return e;
  if (hipError_t e = hipMemsetAsync(O, 0, offsetof(OnsetOut, row), s); e != hipSuccess) return e;
  hipLaunchKernelGGL(onset_scan_kernel, dim3(lat_score_grid(n_sel)), dim3(kLatScoreBlock), 0, s,
                     reinterpret_cast<const ulonglong2 *>(pairs), n_sel, n_cov, OnsetParams{min_count, min_delta, fall},
                     rec, cand, T, O);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  // (no row to sum: the scan took the range's spans)
  if (hipError_t e = launch_top_select(nullptr, 0, k, n_sel, cand, T, s); e != hipSuccess) return e;
  hipLaunchKernelGGL(onset_rows_kernel, dim3((k + kLatQueryBlock - 1) / kLatQueryBlock), dim3(kLatQueryBlock), 0, s, rec,
                     thr_bin, n_sel, T, O);
  return hipGetLastError();
}

}  // namespace sa
