// spanagg_part.hip -- the HBM-table ingest kernels of libspanagg (tables larger
// than LDS): per-span atomics (ingest_hbm_kernel) and the round-1 partitioned
// scatter + aggregate.
#include <algorithm>

#include "sa_device.h"

namespace sa {
namespace {

// ---------------------------------------------------------------------------
// HBM-table path (table larger than LDS): CAS insert + u64 atomics per span;
// 256 threads, 4 spans per lane per tile, no prefetch.  NB >= 0: unrolled for
// NB non-negative bounds; -1: any bounds.
template <int NB>
__global__ __launch_bounds__(kHbmBlock) void ingest_hbm_kernel(IngestParams P) {
  constexpr int S = kHbmSpansPerLane;
  LaneStats st{0, 0, 0, 0};
  const uint32_t nbk = NB >= 0 ? (uint32_t)NB + 1 : P.nbk;
  const uint32_t stride = row_stride(nbk);
  uint64_t lo, hi;
  wg_range(P.n, lo, hi);
  const Cols c = make_cols(P, lo, hi);
  const uint32_t len = (uint32_t)(hi - lo);
  const uint32_t tile = kHbmBlock * S;
  uint32_t off = threadIdx.x * S;
  SpanTile<S> cur;
  load_tile<S>(c, off, len, cur);
  for (uint32_t t0 = 0; t0 < len; t0 += tile, off += tile) {
    SketchPre<S> k;
    sketch_pre<S>(P, cur, k, st);
    uint32_t slot[S], bk[S];
    uint64_t dd[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      slot[j] = kNotFound;
      bk[j] = 0;
      dd[j] = 0;
      if (j < cur.cnt) {
        const uint64_t key = cur.key[j];
        const uint64_t d = cur.e[j] > cur.s[j] ? cur.e[j] - cur.s[j] : 0;
        st.zero_key += key == 0 ? 1u : 0u;
        if (key != 0 && !(P.diag & 1u)) {
          bk[j] = bucket_of<NB>(d, P);
          dd[j] = d;
          const uint32_t found = g_find_insert(P.gkeys, key, P.log2cap, P.max_probe);
          st.dropped += found == kNotFound ? 1u : 0u;
          slot[j] = found;
        }
      }
    }
    // Counter atomics in lane pairs: lanes 2i and 2i+1 each add the count of
    // one span and the sum of the other's, so one instruction carries both
    // cells of a span -- one 64-B segment, one memory-side atomic request
    // (the requests, not the bytes, bound this path: tools/atomic_probe.hip).
    if (!(P.diag & 2048u)) {  // diag 2048: lookups only
      const bool even = (threadIdx.x & 1u) == 0;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const uint32_t os = (uint32_t)__shfl_xor((int)slot[j], 1);
        const uint32_t ob = (uint32_t)__shfl_xor((int)bk[j], 1);
        const uint64_t od = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)dd[j], 1) |
                            ((uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(dd[j] >> 32), 1) << 32);
        // instruction 1: even lane -> its count, odd lane -> the even lane's sum
        const uint32_t s1 = even ? slot[j] : os, b1 = even ? bk[j] : ob;
        if (s1 != kNotFound)
          atomicAdd(P.gcounts + (uint64_t)s1 * stride + (even ? row_count_cell(b1) : row_sum_cell(b1)),
                    even ? 1ULL : (unsigned long long)od);
        // instruction 2: odd lane -> its count, even lane -> the odd lane's sum
        const uint32_t s2 = even ? os : slot[j], b2 = even ? ob : bk[j];
        if (s2 != kNotFound)
          atomicAdd(P.gcounts + (uint64_t)s2 * stride + (even ? row_sum_cell(b2) : row_count_cell(b2)),
                    even ? (unsigned long long)od : 1ULL);
      }
    }
    sketch_post<S>(P, cur, k, slot);
    load_tile<S>(c, off + tile, len, cur);
  }
  flush_stats(P, st);
}

// ---------------------------------------------------------------------------
// Partitioned HBM-table path.  Random per-span lookups and counter atomics
// into a table far larger than LDS bound ingest_hbm_kernel (10 M spans over
// 1 M keys: 552 us).  Here every span is first written as a 16-B record into
// the bin of its key (top 11 bits), then one workgroup per bin aggregates its
// records in an LDS table (~490 keys per bin at 1 M keys) and adds each key's
// row to the HBM counters once, with plain read-modify-write: a key belongs
// to one bin, so its row has one writer per launch.  Records that do not fit
// (a bin beyond its capacity, durations >= 2^57 ns, an LDS table past its
// probe limit) take the direct path: lookup + counter atomics, as in
// ingest_hbm_kernel.  Stats, HLL and ERROR spans are handled in the scatter.

typedef unsigned long long nt_u64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void direct_red(const IngestParams &P, uint64_t key, uint64_t d,
                                           uint32_t bk, uint32_t stride, LaneStats &st) {
  const uint32_t s = g_find_insert(P.gkeys, key, P.log2cap, P.max_probe);
  if (s == kNotFound) {
    st.dropped += 1u;
    return;
  }
  atomicAdd(P.gcounts + (uint64_t)s * stride + row_count_cell(bk), 1ULL);
  atomicAdd(P.gcounts + (uint64_t)s * stride + row_sum_cell(bk), (unsigned long long)d);
}

#ifndef PART_U
#define PART_U 4
#endif
// Records go through a kPartStage-record LDS stage per bin and leave as whole
// chunks (runs are reserved in multiples of kPartStage records, so chunks
// stay aligned).
#ifndef SA_PART_SKIP_USED
#define SA_PART_SKIP_USED 1
#endif
#ifndef SA_PART_WAVES_EU
#define SA_PART_WAVES_EU 1  // 8 caps VGPRs at 64: two 1,024-thread workgroups per CU
#endif
template <int NB>
__global__ __launch_bounds__(kPartBlock, SA_PART_WAVES_EU) void part_scatter_kernel(IngestParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t *cur = reinterpret_cast<uint32_t *>(smem);  // phase 1: counts; then next record index
  uint32_t *lim = cur + kPartBins;                      // end of this workgroup's run in the bin
  uint32_t *scnt = lim + kPartBins;                     // records staged per bin
  ulonglong2 *stage = reinterpret_cast<ulonglong2 *>(scnt + kPartBins);  // [kPartBins][kPartStage]
  unsigned long long *hkey = reinterpret_cast<unsigned long long *>(stage + kPartBins * kPartStage);
  unsigned long long *hsum = hkey + kPartHot;                           // overflow table
  uint32_t *hcnt = reinterpret_cast<uint32_t *>(hsum + kPartHot);       // [kPartHot][kPartMaxBk]
  LaneStats st{0, 0, 0, 0};
  const uint32_t nbk = NB >= 0 ? (uint32_t)NB + 1 : P.nbk;
  const uint32_t stride = row_stride(nbk);
  uint64_t lo, hi;
  wg_range(P.n, lo, hi);
  for (uint32_t b = threadIdx.x; b < kPartBins; b += blockDim.x) cur[b] = scnt[b] = 0;
  for (uint32_t h = threadIdx.x; h < kPartHot; h += blockDim.x) hkey[h] = hsum[h] = 0;
  for (uint32_t h = threadIdx.x; h < kPartHot * kPartMaxBk; h += blockDim.x) hcnt[h] = 0;
  __syncthreads();
  // 1. records per bin in this workgroup's range (key column only; 8 loads
  //    in flight per thread)
  constexpr int U1 = 8;
  for (uint64_t i0 = lo + threadIdx.x; i0 < hi; i0 += (uint64_t)U1 * blockDim.x) {
    uint64_t k[U1];
#pragma unroll
    for (int u = 0; u < U1; ++u) {
      const uint64_t i = i0 + (uint64_t)u * blockDim.x;
      k[u] = i < hi ? P.key[i] : 0;
    }
#pragma unroll
    for (int u = 0; u < U1; ++u)
      if (k[u] != 0) atomicAdd(&cur[part_bin(k[u])], 1u);
  }
  __syncthreads();
  // 2. reserve one contiguous run per bin (one returning atomic per bin)
  for (uint32_t b = threadIdx.x; b < kPartBins; b += blockDim.x) {
    const uint32_t c = (cur[b] + kPartStage - 1) & ~(kPartStage - 1);
    uint32_t base = 0;
    if (c) base = atomicAdd(&P.part_fill[b], c);
    const uint64_t b0 = (uint64_t)b * P.part_cap;
    cur[b] = (uint32_t)(b0 + min(base, P.part_cap));
    lim[b] = (uint32_t)(b0 + min(base + c, P.part_cap));
  }
  __syncthreads();
  // a span whose bin run is full: into the overflow table (hot keys of a
  // skewed mix overfill their bins; per-span global atomics on one row would
  // serialise), else the direct path
  auto spill = [&](uint64_t key, uint64_t d, uint32_t bk) {
    uint32_t h = ((uint32_t)key * 0x9E3779B1u) >> (32 - kPartHotBits);
    for (int pr = 0; pr < 8; ++pr, h = (h + 1) & (kPartHot - 1)) {
      unsigned long long k = hkey[h];
      if (k == 0) k = atomicCAS(&hkey[h], 0ULL, (unsigned long long)key);
      if (k == 0 || k == key) {
        atomicAdd(&hcnt[h * kPartMaxBk + bk], 1u);
        atomicAdd(&hsum[h], (unsigned long long)d);
        return;
      }
    }
    direct_red(P, key, d, bk, stride, st);
  };
  auto put = [&](uint32_t b, const ulonglong2 &rec, uint64_t d, uint32_t bk) {  // one record, now
    const uint32_t r = atomicAdd(&cur[b], 1u);
    if (r < lim[b]) P.part_rec[r] = rec;  // write-back: partial lines merge in L2
    else spill(rec.x, d, bk);
  };
  // 3. every span: stats, sketches, and its record (or the direct path);
  //    U spans per thread with all their loads issued first; rounds are
  //    workgroup-uniform (the stages are flushed between them)
  constexpr int U = PART_U;
  for (uint64_t r0 = lo; r0 < hi; r0 += (uint64_t)U * blockDim.x) {
   const uint64_t i0 = r0 + threadIdx.x;
   uint64_t K[U], S0[U], E0[U], A[U], B[U];
   uint32_t M[U];
#pragma unroll
   for (int u = 0; u < U; ++u) {
     const uint64_t i = i0 + (uint64_t)u * blockDim.x;
     const bool ok = i < hi;
     K[u] = ok ? P.key[i] : 0;
     S0[u] = ok ? P.start[i] : 0;
     E0[u] = ok ? P.end[i] : 0;
     A[u] = ok ? P.w0[i] : 0;
     B[u] = ok ? P.w1[i] : 0;
     M[u] = ok ? P.meta[i] : 0xFFFFu;  // padding lanes are skipped below
   }
   // sketch phase A for all U spans: the HLL register reads are issued
   // together (unconditional: a skipped span reads the first byte)
   uint32_t WS[U], RHO[U], CUR[U];
   uint8_t *REG[U];
#pragma unroll
   for (int u = 0; u < U; ++u) {
    const bool in = i0 + (uint64_t)u * blockDim.x < hi;
    const uint32_t svc = M[u] & 0xFFFFu;
    const bool svc_ok = svc < P.n_services;
    const uint64_t win = fast_div(E0[u], P.window_ns, P.win_magic);
    const bool win_ok = win - P.win_base < (uint64_t)P.n_windows;
    if (in) {
      st.zero_key += K[u] == 0 ? 1u : 0u;
      st.bad_svc += svc_ok ? 0u : 1u;
      st.oor += (svc_ok && !win_ok) ? 1u : 0u;
    }
    WS[u] = in && svc_ok && win_ok ? (uint32_t)(win & P.win_mask) : 0xFFFFFFFFu;
    RHO[u] = 0;
    REG[u] = P.hll;
    if (WS[u] != 0xFFFFFFFFu && !(P.diag & 2u)) {
      const uint64_t x = xxh64_16(A[u], B[u]);
      RHO[u] = (uint32_t)__clzll((long long)((x << P.p) | (1ULL << (P.p - 1)))) + 1;
      REG[u] = P.hll + ((((uint64_t)WS[u] * P.n_services + svc) << P.p) + (x >> (64 - P.p)));
    }
   }
#pragma unroll
   for (int u = 0; u < U; ++u) CUR[u] = *REG[u];
#pragma unroll
   for (int u = 0; u < U; ++u) {
    if (i0 + (uint64_t)u * blockDim.x >= hi) continue;
    const uint64_t key = K[u], s0 = S0[u], e0 = E0[u];
    const uint32_t meta = M[u];
    const uint64_t d = e0 > s0 ? e0 - s0 : 0;
    const uint32_t bk = bucket_of<NB>(d, P);
    const uint32_t ws = WS[u];
    if (key != 0 && !(P.diag & 1u)) {
      const uint32_t b = part_bin(key);
      const ulonglong2 rec = make_ulonglong2(key, (d << 7) | bk);
      if (d >= (1ULL << 57)) {
        direct_red(P, key, d, bk, stride, st);
      } else if (SA_PART_SKIP_USED && cur[b] >= lim[b]) {  // run used up (stays so): no stage, no cur atomic
        spill(key, d, bk);
      } else {
        const uint32_t slot = atomicAdd(&scnt[b], 1u);
        if (slot < kPartStage) stage[b * kPartStage + slot] = rec;
        else put(b, rec, d, bk);
      }
    }
    // ERROR spans: the exact per-(window, slot) counter (count-min cells are
    // folded from it); no slot (key 0, table full): the cells directly
    if (ws != 0xFFFFFFFFu && ((meta >> 19) & 3u) == 2u && !(P.diag & 4u)) {
      const uint32_t slot = key != 0 ? g_find_insert(P.gkeys, key, P.log2cap, P.max_probe) : kNotFound;
      if (slot != kNotFound) atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + slot, 1ULL);
      else cms_add(P, ws, key, 1ULL);
    }
   }
#pragma unroll
   for (int u = 0; u < U; ++u)
     if ((CUR[u] & 0xFFu) < RHO[u]) hll_raise(REG[u], RHO[u]);
   // full stages leave as one chunk
   __syncthreads();
   for (uint32_t b = threadIdx.x; b < kPartBins; b += blockDim.x) {
     if (scnt[b] < kPartStage) continue;
     const uint32_t r = cur[b];
     cur[b] = r + kPartStage;
     scnt[b] = 0;
#pragma unroll
     for (int j = 0; j < (int)kPartStage; ++j) {
       const ulonglong2 rec = stage[b * kPartStage + j];
       if (r + j < lim[b]) P.part_rec[r + j] = rec;
       else spill(rec.x, rec.y >> 7, (uint32_t)(rec.y & 127u));
     }
   }
   __syncthreads();
  }
  // partial stages, then zero records over the run's unused tail (the
  // padding, and the slots of spans that took the direct path)
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < kPartBins; b += blockDim.x) {
    for (uint32_t j = 0; j < scnt[b]; ++j) {
      const ulonglong2 rec = stage[b * kPartStage + j];
      put(b, rec, rec.y >> 7, (uint32_t)(rec.y & 127u));
    }
    for (uint32_t r = cur[b]; r < lim[b]; ++r) P.part_rec[r] = make_ulonglong2(0, 0);
  }
  // the overflow table: one atomic per non-zero cell per key (the aggregate
  // kernel's plain row updates come after this kernel)
  __syncthreads();
  for (uint32_t h = threadIdx.x; h < kPartHot; h += blockDim.x) {
    const unsigned long long key = hkey[h];
    if (key == 0) continue;
    const uint32_t g = g_find_insert(P.gkeys, key, P.log2cap, P.max_probe);
    if (g == kNotFound) {
      for (uint32_t b = 0; b < nbk; ++b) st.dropped += hcnt[h * kPartMaxBk + b];
      continue;
    }
    unsigned long long *row = P.gcounts + (uint64_t)g * stride;
    for (uint32_t b = 0; b < nbk; ++b)
      if (const uint32_t c = hcnt[h * kPartMaxBk + b]) atomicAdd(row + row_count_cell(b), (unsigned long long)c);
    atomicAdd(row + row_sum_cell(0), hsum[h]);
  }
  flush_stats(P, st);
}

// One workgroup per bin: LDS table of kPartSlots keys (linear probing from a
// hash of the key's low bits; the bin fixes its top bits), u16 bucket-count
// pairs (a bin holds < 2^16 records) and u64 ns sums -- 52 KiB, three
// workgroups per CU -- then one read-modify-write of each key's HBM row.
__global__ __launch_bounds__(kPartAggBlock) void part_aggregate_kernel(IngestParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long *lkeys = reinterpret_cast<unsigned long long *>(smem);
  unsigned long long *lsum = lkeys + kPartSlots;
  uint32_t *lcnt = reinterpret_cast<uint32_t *>(lsum + kPartSlots);  // [kPartSlots][kPartWords]
  const uint32_t nbk = P.nbk, stride = row_stride(nbk);
  auto cnt = [&](uint32_t s, uint32_t b) -> uint32_t {
    return (lcnt[s * kPartWords + (b >> 1)] >> ((b & 1u) * 16)) & 0xFFFFu;
  };
  LaneStats st{0, 0, 0, 0};
  __shared__ uint32_t spilled;  // direct-path atomics from this workgroup
  if (threadIdx.x == 0) spilled = 0;
  const uint32_t bin = blockIdx.x;
  const uint32_t n = (P.diag & 1u) ? 0u : min(P.part_fill[bin], P.part_cap);  // diag 1: no records
  for (uint32_t i = threadIdx.x; i < kPartSlots; i += blockDim.x) lkeys[i] = lsum[i] = 0;
  for (uint32_t i = threadIdx.x; i < kPartSlots * kPartWords; i += blockDim.x) lcnt[i] = 0;
  __syncthreads();
  const ulonglong2 *rec = P.part_rec + (uint64_t)bin * P.part_cap;
  constexpr int R = 8;  // records in flight per thread
  for (uint32_t i0 = 0; i0 < n; i0 += R * blockDim.x) {
    ulonglong2 v[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const uint32_t i = i0 + u * blockDim.x + threadIdx.x;
      v[u] = i < n ? rec[i] : make_ulonglong2(0, 0);
    }
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const unsigned long long key = v[u].x;
      if (key == 0) continue;
      const uint64_t d = v[u].y >> 7;
      const uint32_t bk = (uint32_t)(v[u].y & 127u);
      uint32_t s = ((uint32_t)key * 0x9E3779B1u) >> (32 - kPartSlotBits), found = kNotFound;
      for (int pr = 0; pr < 64; ++pr, s = (s + 1) & (kPartSlots - 1)) {
        unsigned long long k = lkeys[s];
        if (k == 0) k = atomicCAS(&lkeys[s], 0ULL, key);
        if (k == 0 || k == key) {
          found = s;
          break;
        }
      }
      if (found != kNotFound) {
        atomicAdd(&lcnt[found * kPartWords + (bk >> 1)], 1u << ((bk & 1u) * 16));
        atomicAdd(&lsum[found], (unsigned long long)d);
      } else {
        direct_red(P, key, d, bk, stride, st);
        spilled = 1;
      }
    }
  }
  __syncthreads();
  // Row updates below use plain loads: a row belongs to this workgroup's bin,
  // so in this launch only this workgroup writes it (earlier launches' writes
  // are visible at the kernel boundary).  After a direct-path spill the
  // row may also hold this launch's atomics, which are performed beyond the
  // XCD's L2: then fence and read at agent scope.
  const bool coherent = spilled != 0;
  if (coherent) {
    __threadfence();
    __syncthreads();
  }
  if (threadIdx.x == 0) P.part_fill[bin] = 0;  // ready for the next launch
  for (uint32_t s = threadIdx.x; s < kPartSlots && !(P.diag & 8u); s += blockDim.x) {
    const unsigned long long key = lkeys[s];
    if (key == 0) continue;
    // the key's first-choice bucket in four independent loads (most keys sit
    // there); the full probe sequence only for the rest
    const ProbeSeq pr = probe_seq(key, P.log2cap);
    const ulonglong2 *bq = reinterpret_cast<const ulonglong2 *>(P.gkeys + pr.b1 * 4);
    const ulonglong2 qa = bq[0], qb = bq[1];  // stale reads just miss: see g_find_insert
    const unsigned long long q[4] = {qa.x, qa.y, qb.x, qb.y};
    uint32_t g = kNotFound;
#pragma unroll
    for (int j = 3; j >= 0; --j) g = q[j] == key ? pr.b1 * 4 + j : g;
    if (g == kNotFound) g = g_find_insert(P.gkeys, key, P.log2cap, P.max_probe);
    if (g == kNotFound) {
      uint32_t calls = 0;
      for (uint32_t b = 0; b < nbk; ++b) calls += cnt(s, b);
      st.dropped += calls;
      continue;
    }
    unsigned long long *row = P.gcounts + (uint64_t)g * stride;
    // every load issued before any store (no wait per cell)
    unsigned long long old[kPartMaxBk + 1];
    if (coherent) {
#pragma unroll
      for (uint32_t b = 0; b < kPartMaxBk; ++b)  // unconditional (in-row address), no branch per load
        old[b] = __hip_atomic_load(row + (b < nbk ? row_count_cell(b) : 0u), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
      old[kPartMaxBk] = __hip_atomic_load(row + row_sum_cell(0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      // the row's (<= 3) 64-B segments as 16-B loads
      constexpr uint32_t kSeg = (kPartMaxBk + kSegBuckets - 1) / kSegBuckets;
      const uint32_t nseg = stride / 8;
      ulonglong2 v[kSeg * 4];
#pragma unroll
      for (uint32_t k = 0; k < kSeg * 4; ++k)
        v[k] = reinterpret_cast<const ulonglong2 *>(row)[(k / 4 < nseg ? k : k % 4)];
      auto cell = [&](uint32_t c) -> unsigned long long { return (c & 1u) ? v[c / 2].y : v[c / 2].x; };
#pragma unroll
      for (uint32_t b = 0; b < kPartMaxBk; ++b) old[b] = b < nbk ? cell(row_count_cell(b)) : 0ULL;
      old[kPartMaxBk] = cell(row_sum_cell(0));
    }
#pragma unroll
    for (uint32_t b = 0; b < kPartMaxBk; ++b)
      if (b < nbk && cnt(s, b)) row[row_count_cell(b)] = old[b] + cnt(s, b);
    row[row_sum_cell(0)] = old[kPartMaxBk] + lsum[s];
  }
  flush_stats(P, st);
}

}  // namespace

hipError_t launch_ingest_part(const IngestParams &P, hipStream_t s) {
  const uint32_t grid = (uint32_t)std::min<uint64_t>(kPartMaxGrid, (P.n + kPartBlock - 1) / kPartBlock);
  const void *fn = bounds16(P.nneg, P.npos) ? (const void *)&part_scatter_kernel<16> : (const void *)&part_scatter_kernel<-1>;
  void *args[] = {const_cast<IngestParams *>(&P)};
  if (hipError_t e = hipLaunchKernel(fn, dim3(grid), dim3(kPartBlock), args, kPartScatterLds, s); e != hipSuccess)
    return e;
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(part_aggregate_kernel, dim3(kPartBins), dim3(kPartAggBlock), kPartLdsBytes, s, P);
  return hipGetLastError();
}

hipError_t prepare_ingest_part() {
  for (const void *fn : {(const void *)&part_scatter_kernel<16>, (const void *)&part_scatter_kernel<-1>})
    if (hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPartScatterLds);
        e != hipSuccess)
      return e;
  return hipFuncSetAttribute((const void *)&part_aggregate_kernel,
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kPartLdsBytes);
}

hipError_t launch_ingest_hbm(const IngestParams &P, uint32_t grid, hipStream_t s) {
  if (bounds16(P.nneg, P.npos)) hipLaunchKernelGGL(ingest_hbm_kernel<16>, dim3(grid), dim3(kHbmBlock), 0, s, P);
  else hipLaunchKernelGGL(ingest_hbm_kernel<-1>, dim3(grid), dim3(kHbmBlock), 0, s, P);
  return hipGetLastError();
}

}  // namespace sa
