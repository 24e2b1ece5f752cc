// spanagg_kernels.hip -- CDNA4 (gfx950) kernels of libspanagg.
//
// One fused streaming pass per span batch replaces the connector's per-span
// body ([UPSTREAM] spanmetricsconnector connector.go `aggregateMetrics`:
// duration, buildKey -> map lookup, Sum.Add(1), explicitHistogram.Observe;
// SURVEY.md 3A step 5) and adds the per-service HLL / error count-min updates
// (SURVEY.md Appendix C).  Memory- and atomic-bound, no MFMA:
//   * coalesced SoA reads, 2 spans per lane (16-B loads per column);
//   * duration -> bucket by u64 compares against host-derived integer
//     thresholds (exactly SearchFloat64s(bounds, float64(d)/1e6));
//   * small-table path: the HBM key table is mirrored in LDS (same slots), and
//     per-workgroup LDS u16 counters + u64 ns sums are flushed, every epoch of
//     <= 65535 spans, into a workgroup-private HBM slab with plain
//     read-modify-write (no global atomics on the hot path); the slabs are
//     summed only at flush time (reduce kernel);
//   * HBM-table path (high cardinality): lock-free CAS insert + u64 atomics;
//   * HLL: u8 registers in HBM, read-filtered, CAS-max only when rho grows;
//   * count-min: u64 cells, atomic add per ERROR span per row.
// (the HBM-table kernels: spanagg_part.hip; the flush-time table kernels:
// spanagg_table.hip)
#include "sa_device.h"

namespace sa {
namespace {

// ---------------------------------------------------------------------------
// Small-table path.  LDS layout (dynamic, 16-B aligned; sa_path.h
// small_lds_layout lists the regions and sizes the launch from them):
//   lkeys [cap] u64   mirror of the HBM key table (same slot positions)
//   lsum  [cap] u64   per-slot ns sum of this epoch
//   lcnt  [cap][nw] u32, nw = ceil(nbk/2): two u16 bucket counters per word
//   hq    [kHllQueue] (hoff, rho) deferred HLL raises
//   hq_n  [4] the queue's fill, the next chunk claim, the filtered HLL updates
//   lstat [4] LEAN event counts (zero key, bad service, out of ring, dropped)
//   lbins [kBins] bucket bin table
//   etab  [kErrTab] (key + 1) << 16 | count of the ERROR spans
//   llb   [kLbMaxSub] HLL lower bounds
//   lsc   [cap] EXPO with index records: each slot's scale at the kernel's start
// (ingest_lds_kernel uses lkeys .. hq_n[0])
struct SmallLds {
  unsigned long long *lkeys, *lsum;
  uint32_t *lcnt;
  uint2 *hq;
  uint32_t *hq_n, *lstat;
  BinEntry *lbins;
  uint32_t *etab;
  uint8_t *llb;
  int8_t *lsc;
};
// Each pointer starts where the one before ends: typed pointer arithmetic over
// the host list's element counts (the compiler folds this form best).
__device__ __forceinline__ SmallLds small_lds_carve(unsigned char *smem, uint32_t cap, uint32_t nw, bool expo) {
  const SmallLdsLayout R = small_lds_layout(cap, nw, expo);
  auto n = [&](int region) { return (uint32_t)R.r[region].n; };
  SmallLds L;
  L.lkeys = reinterpret_cast<unsigned long long *>(smem);
  L.lsum = L.lkeys + n(kLdsKeys);
  L.lcnt = reinterpret_cast<uint32_t *>(L.lsum + n(kLdsSums));
  L.hq = reinterpret_cast<uint2 *>(L.lcnt + n(kLdsCnt));
  L.hq_n = reinterpret_cast<uint32_t *>(L.hq + n(kLdsHq));
  L.lstat = L.hq_n + 4;  // the control block's second half
  L.lbins = reinterpret_cast<BinEntry *>(L.hq_n + n(kLdsCtl));
  L.etab = reinterpret_cast<uint32_t *>(L.lbins + n(kLdsBins));
  L.llb = reinterpret_cast<uint8_t *>(L.etab + n(kLdsErr));
  L.lsc = reinterpret_cast<int8_t *>(L.llb + n(kLdsLb));
  return L;
}
// The carve ends where the host's size does (SmallLdsLayout::end) when every
// step is as wide as the list says: for any geometry, so for the compile-time
// ones (LC 11 / NWC 9, the EXPO LC 11) too.  lsc + its count + the reserved
// tail is the end; nothing is carved after it.
constexpr bool small_lds_steps_match() {
  constexpr SmallLdsLayout R = small_lds_layout(1u << 11, 9, true);
  return sizeof(*SmallLds{}.lkeys) == R.r[kLdsKeys].elem && sizeof(*SmallLds{}.lsum) == R.r[kLdsSums].elem &&
         sizeof(*SmallLds{}.lcnt) == R.r[kLdsCnt].elem && sizeof(*SmallLds{}.hq) == R.r[kLdsHq].elem &&
         sizeof(*SmallLds{}.hq_n) == R.r[kLdsCtl].elem && sizeof(*SmallLds{}.lbins) == R.r[kLdsBins].elem &&
         sizeof(*SmallLds{}.etab) == R.r[kLdsErr].elem && sizeof(*SmallLds{}.llb) == R.r[kLdsLb].elem &&
         sizeof(*SmallLds{}.lsc) == R.r[kLdsScale].elem && kLdsScale + 2 == kLdsRegions;
}
static_assert(small_lds_steps_match(), "small_lds_carve's pointer types vs. sa_path.h small_lds_layout");
static_assert(small_lds_layout(1u << 11, 9, false).end() == 2048 * 52 + kLdsExtraBytes &&
                  small_lds_layout(1u << 11, kExpoWords, true).end() == 2048 * 41 + kLdsExtraBytes,
              "the compile-time geometries' LDS");

// The workgroup's HBM slab is [cap][2*nw] u32 (+ [cap] u64 sums): LDS word w
// maps to slab cells 2w and 2w+1, so a pair of LDS words is one 16-B slab
// vector and the flush is a vectorised read-modify-write of touched cells.
__device__ __forceinline__ void flush_lds(const IngestParams &P, uint32_t cap, uint32_t nw,
                                          unsigned long long *lsum, uint32_t *lcnt) {
  if (P.diag & 8u) return;
  uint4 *scnt = reinterpret_cast<uint4 *>(P.slab_cnt + (uint64_t)blockIdx.x * cap * 2 * nw);
  uint2 *lw = reinterpret_cast<uint2 *>(lcnt);
  const uint32_t pairs = cap * nw / 2;
  constexpr int U = 5;  // two rounds of loads for cap 2048 x nw 9 at 1,024 threads
  for (uint32_t k0 = threadIdx.x; k0 < pairs; k0 += U * blockDim.x) {
    uint2 w[U];
    uint4 g[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t k = k0 + u * blockDim.x;
      w[u] = k < pairs ? lw[k] : make_uint2(0, 0);
      g[u] = (w[u].x | w[u].y) ? scnt[k] : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t k = k0 + u * blockDim.x;
      if (w[u].x | w[u].y) {
        g[u].x += w[u].x & 0xFFFFu;
        g[u].y += w[u].x >> 16;
        g[u].z += w[u].y & 0xFFFFu;
        g[u].w += w[u].y >> 16;
        scnt[k] = g[u];
        lw[k] = make_uint2(0, 0);
      }
    }
  }
  ulonglong2 *ss = reinterpret_cast<ulonglong2 *>(P.slab_sum + (uint64_t)blockIdx.x * cap);
  ulonglong2 *ls = reinterpret_cast<ulonglong2 *>(lsum);
  for (uint32_t k = threadIdx.x; k < cap / 2; k += blockDim.x) {
    const ulonglong2 v = ls[k];
    if (v.x | v.y) {
      ulonglong2 g = ss[k];
      g.x += v.x;
      g.y += v.y;
      ss[k] = g;
      ls[k] = make_ulonglong2(0, 0);
    }
  }
}

// End-of-launch write-back of ingest_v2_kernel for a compile-time geometry
// (UPT slab-count pairs and SPT slab-sum pairs per thread), in two phases.
//
// v2_epi_pre runs in each wave right after its own loop, before the
// workgroup barrier: it loads the thread's slab-count and slab-sum words (all
// of them: which ones the launch touched is known only after the barrier) and
// the lower-bound sub-block of its wave.  The slabs are this workgroup's own
// (no other workgroup of the launch writes them; the previous launch of the
// slab set has completed), and a stale register read for the bound can only
// lower it, which keeps it a lower bound.  Waves end their loops up to ~10 us
// apart, so these loads land while the last waves still work.
//
// v2_epilogue runs after the barrier: LDS counters plus the prefetched words
// -> dependent stores of the touched words, the ERROR counts as no-return
// atomics on the workgroup's private ERROR slab, and the queued HLL raises as
// CAS from the register word each span saw in the loop (queued beside it), so
// the only memory round trip left after the barrier is a raise's CAS (one
// more when another workgroup changed the word since).  Before, the slab, ERROR
// and HLL words were read after the barrier: two round trips.  (The EXPO
// kernel's epilogue shares the raise and bound halves.)

// After the barrier: the queued HLL raises, each a CAS from the register word
// its span saw in the loop (hqv), and the bound from the prefetched quads.
template <uint32_t B, uint32_t Q, typename PT>
__device__ __forceinline__ void epi_raise_and_bound(const PT &P, const uint2 *hq, const uint32_t *hqv, uint32_t nq,
                                                    const uint4 (&lv)[4]) {
  const uint32_t tid = threadIdx.x;
  constexpr uint32_t kQ = Q / B;
#pragma unroll
  for (uint32_t i = 0; i < kQ; ++i) {
    if (tid + i * B >= nq) continue;
    const uint2 q = hq[tid + i * B];
    SA_GLOBAL uint32_t *word = gbl(reinterpret_cast<uint32_t *>(P.hll + (q.x & ~3u)));
    hll_raise_from(word, hqv[tid + i * B], (q.x & 3u) * 8, q.y);
  }
  hll_lb_finish<B>(P, lv);
}

// This workgroup's LDS ERROR table -> its private ERROR slab (kErrTab / B
// entries per thread).  ATOMIC: no-return atomics, for the epilogues whose
// other stores are already in flight; otherwise a plain read-modify-write.
template <uint32_t B, bool ATOMIC, typename PT>
__device__ __forceinline__ void errtab_to_slab(const PT &P, const uint32_t *etab, bool err_lds, uint32_t log2cap) {
  if (!err_lds) return;
  for (uint32_t t = threadIdx.x; t < kErrTab; t += B) {
    const uint32_t e = etab[t];
    if (e) {
      uint32_t *cell = P.errslab + (uint64_t)blockIdx.x * ((uint64_t)P.n_windows << log2cap) + ((e >> 16) - 1);
      if constexpr (ATOMIC) atomicAdd(cell, e & 0xFFFFu);
      else *cell += e & 0xFFFFu;
    }
  }
}

template <int UPT, int SPT>
struct EpiPre {
  uint4 g[UPT];
  ulonglong2 sg[SPT];
  uint4 lv[4];
};

template <int UPT, int SPT, uint32_t B, typename PT>
__device__ __forceinline__ void v2_epi_pre(const PT &P, uint32_t cap, uint32_t nw, EpiPre<UPT, SPT> &x) {
  const uint32_t tid = threadIdx.x;
  const uint4 *scnt = reinterpret_cast<const uint4 *>(P.slab_cnt + (uint64_t)blockIdx.x * cap * 2 * nw);
#pragma unroll
  for (int u = 0; u < UPT; ++u) x.g[u] = scnt[tid + u * B];
  const ulonglong2 *ss = reinterpret_cast<const ulonglong2 *>(P.slab_sum + (uint64_t)blockIdx.x * cap);
#pragma unroll
  for (int u = 0; u < SPT; ++u) x.sg[u] = ss[tid + u * B];
  hll_lb_pre<B>(P, x.lv);
}

template <int UPT, int SPT, uint32_t B, uint32_t Q, typename PT>
__device__ __forceinline__ void v2_epilogue(const PT &P, uint32_t cap, uint32_t nw, uint32_t log2cap,
                                            const unsigned long long *lsum, const uint32_t *lcnt,
                                            const uint32_t *etab, bool err_lds, const uint2 *hq,
                                            const uint32_t *hqv, uint32_t nq, const EpiPre<UPT, SPT> &x) {
  const uint32_t tid = threadIdx.x;
  const bool slabs = !(P.diag & 8u);
  uint4 *scnt = reinterpret_cast<uint4 *>(P.slab_cnt + (uint64_t)blockIdx.x * cap * 2 * nw);
  const uint2 *lw = reinterpret_cast<const uint2 *>(lcnt);
#pragma unroll
  for (int u = 0; u < UPT; ++u) {
    const uint2 w = slabs ? lw[tid + u * B] : make_uint2(0, 0);
    if (w.x | w.y) {
      uint4 g = x.g[u];
      g.x += w.x & 0xFFFFu;
      g.y += w.x >> 16;
      g.z += w.y & 0xFFFFu;
      g.w += w.y >> 16;
      scnt[tid + u * B] = g;
    }
  }
  ulonglong2 *ss = reinterpret_cast<ulonglong2 *>(P.slab_sum + (uint64_t)blockIdx.x * cap);
  const ulonglong2 *ls = reinterpret_cast<const ulonglong2 *>(lsum);
#pragma unroll
  for (int u = 0; u < SPT; ++u) {
    const ulonglong2 sv = slabs ? ls[tid + u * B] : make_ulonglong2(0, 0);
    if (sv.x | sv.y) ss[tid + u * B] = make_ulonglong2(x.sg[u].x + sv.x, x.sg[u].y + sv.y);
  }
  errtab_to_slab<B, true>(P, etab, err_lds, log2cap);
  epi_raise_and_bound<B, Q>(P, hq, hqv, nq, x.lv);
}

// Probe the LDS key mirror along the key's sequence from position i0 (the
// earlier positions are known not to hold `key`); returns the slot or
// kNotFound (empty slot reached / probe limit).
__device__ __forceinline__ uint32_t lds_probe_rest(const unsigned long long *lkeys, uint64_t key,
                                                   uint32_t log2cap, uint32_t i0,
                                                   uint32_t max_probe) {
  const ProbeSeq pr = probe_seq(key, log2cap);
  for (uint32_t i = i0; i < max_probe; ++i) {
    const uint32_t s = seq_slot(pr, i);
    const unsigned long long kk = lkeys[s];
    if (kk == key) return s;
    if (kk == 0) break;
  }
  return kNotFound;
}

// Small-table path (key table mirrored in LDS) for bounds no bin table holds:
// buckets by linear thresholds, 1,024 threads, 4 spans per lane per tile.
// Per tile:
//   1. wait for the tile, compact it to (key, duration, bucket, HLL offset,
//      rho, window slot) -- the raw 44 B/span registers are then free;
//   2. 4 LDS key probes back to back -> key-table slots;
//   3. ERROR spans: one no-return atomic on the exact (window, slot) counter;
//   4. issue the 4 HLL register reads;
//   5. prefetch the next tile into the freed tile registers, then the LDS
//      counter / sum atomics;
//   6. HLL compare (a counted vmcnt: the prefetch stays in flight); a register
//      that grows is queued in LDS and raised after the loop, so no returning
//      global atomic (and its vmcnt(0)) sits in the loop.
// LDS: lkeys[cap] u64 | lsum[cap] u64 | lcnt[cap][nw] u32 | hq[kHllQueue] u64 |
//      hq_n (16 B)
__global__ __launch_bounds__(kLdsBlock) void ingest_lds_kernel(IngestParams P) {
  constexpr int S = 4;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t cap = 1u << P.log2cap;
  const uint32_t nbk = P.nbk;
  const uint32_t nw = (nbk + 1) >> 1;
  const SmallLds L = small_lds_carve(smem, cap, nw, false);  // (the head: lkeys .. hq_n[0])
  unsigned long long *const lkeys = L.lkeys, *const lsum = L.lsum;
  uint32_t *const lcnt = L.lcnt, *const hq_n = L.hq_n;
  uint2 *const hq = L.hq;

  uint64_t lo, hi;
  wg_range(P.n, lo, hi);
  const Cols c = make_cols(P, lo, hi);
  const uint32_t len = (uint32_t)(hi - lo);
  const uint32_t tile = kLdsBlock * S;
  uint32_t off = threadIdx.x * S;

  // Key-table loads first, then the first tile's loads: the LDS setup waits
  // only for the keys (vmcnt counts in issue order).
  unsigned long long kv[8];
  const uint32_t per = (cap + kLdsBlock - 1) / kLdsBlock;  // <= 8 for cap <= 8192
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const uint32_t i = threadIdx.x + u * kLdsBlock;
    kv[u] = (u < (int)per && i < cap)
                ? __hip_atomic_load(&P.gkeys[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                : 0ULL;
  }
  SpanTile<S> cur;
  load_tile<S>(c, off, len, cur);
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const uint32_t i = threadIdx.x + u * kLdsBlock;
    if (u < (int)per && i < cap) {
      lkeys[i] = kv[u];
      lsum[i] = 0;
    }
  }
  for (uint32_t i = threadIdx.x; i < cap * nw; i += kLdsBlock) lcnt[i] = 0;
  if (threadIdx.x == 0) *hq_n = 0;
  __syncthreads();

  LaneStats st{0, 0, 0, 0};
  uint32_t in_epoch = 0;
  for (uint32_t t0 = 0; t0 < len; t0 += tile, off += tile) {
    // 1. compact the landed tile; info = bucket | rho << 6 | err << 13 | ws << 14
    //    (bucket < 64, rho <= 65, ws < 4096 window slots)
    uint64_t key[S], dur[S];
    uint32_t hoff[S], info[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool valid = j < cur.cnt;
      key[j] = valid ? cur.key[j] : 0;
      st.zero_key += (valid && cur.key[j] == 0) ? 1u : 0u;
      dur[j] = cur.e[j] > cur.s[j] ? cur.e[j] - cur.s[j] : 0;
      const uint32_t bkt = bucket_of<-1>(dur[j], P);
      const uint32_t svc = cur.meta[j] & 0xFFFFu;
      const bool svc_ok = svc < P.n_services;
      const uint32_t ws = window_slot(P, cur.e[j]);
      const bool win_ok = ws != 0xFFFFFFFFu;
      st.bad_svc += (valid && !svc_ok) ? 1u : 0u;
      st.oor += (valid && svc_ok && !win_ok) ? 1u : 0u;
      const bool sk = valid && svc_ok && win_ok;
      const uint32_t err = (sk && ((cur.meta[j] >> 19) & 3u) == 2u) ? 1u : 0u;
      uint32_t rho = 0;
      hoff[j] = 0;
      if (sk) {
        const uint64_t x = xxh64_16(cur.a[j], cur.b[j]);
        rho = (uint32_t)__clzll((long long)((x << P.p) | (1ULL << (P.p - 1)))) + 1;
        hoff[j] = (((ws * P.n_services + svc) << P.p) + (uint32_t)(x >> (64 - P.p)));
      }
      info[j] = bkt | (rho << 6) | (err << 13) | ((ws & 4095u) << 14);
    }
    // 2. RED lookup: S LDS probes back to back (key no longer needed after)
    uint32_t found[S];
    uint32_t sl[S];
    unsigned long long k0[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      sl[j] = probe_seq(key[j], P.log2cap).b1 * 4;
      k0[j] = lkeys[sl[j]];
    }
#pragma unroll
    for (int j = 0; j < S; ++j) {
      found[j] = kNotFound;
      if (key[j] != 0) {
        found[j] = k0[j] == key[j] ? sl[j]
                   : k0[j] == 0    ? kNotFound
                                   : lds_probe_rest(lkeys, key[j], P.log2cap, 1, P.max_probe);
        if (found[j] == kNotFound) {
          found[j] = g_find_insert(P.gkeys, key[j], P.log2cap, P.max_probe);
          if (found[j] != kNotFound) lkeys[found[j]] = key[j];
        }
        st.dropped += found[j] == kNotFound ? 1u : 0u;
      }
    }
    // 3. error counts: exact per (window, slot) -- one no-return atomic,
    //    issued before the prefetch so the loop-top wait never covers it;
    //    spans without a slot update the count-min cells directly
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (info[j] & (1u << 13)) {
        if (found[j] != kNotFound)
          atomicAdd(P.errcnt + (((uint64_t)(info[j] >> 14)) << P.log2cap) + found[j], 1ULL);
        else
          cms_add(P, info[j] >> 14, key[j], 1ULL);
      }
    }
    // 4. HLL register reads (unconditional: offset 0 when unused)
    uint32_t hv[S];
#pragma unroll
    for (int j = 0; j < S; ++j)
      hv[j] = *reinterpret_cast<const uint32_t *>(P.hll + (hoff[j] & ~3u));
    // 5. prefetch the next tile
    __builtin_amdgcn_sched_barrier(0);
    load_tile<S>(c, off + tile, len, cur);
    __builtin_amdgcn_sched_barrier(0);
    // 5b. RED update: LDS u16 bucket counter + u64 ns sum
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (found[j] != kNotFound) {
        const uint32_t b = info[j] & 63u;
        atomicAdd(&lcnt[found[j] * nw + (b >> 1)], 1u << ((b & 1) * 16));
        atomicAdd(&lsum[found[j]], (unsigned long long)dur[j]);
      }
    }
    // 6. HLL: queue the registers that grow
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const uint32_t rho = (info[j] >> 6) & 127u;
      if (((hv[j] >> ((hoff[j] & 3u) * 8)) & 0xFFu) < rho) {  // (hv: the aligned word the register lies in)
        const uint32_t q = atomicAdd(hq_n, 1u);
        if (q < kHllQueue) hq[q] = make_uint2(hoff[j], rho);
        else hll_raise(P.hll + hoff[j], rho);
      }
    }
    if (++in_epoch == P.epoch_tiles) {  // u16 LDS counters: flush before they can wrap
      __syncthreads();
      flush_lds(P, cap, nw, lsum, lcnt);
      __syncthreads();
      in_epoch = 0;
    }
  }
  __syncthreads();
  flush_lds(P, cap, nw, lsum, lcnt);
  const uint32_t nq = *hq_n < kHllQueue ? *hq_n : kHllQueue;
  for (uint32_t i = threadIdx.x; i < nq; i += kLdsBlock) hll_raise(P.hll + hq[i].x, hq[i].y);
  flush_stats(P, st);
}

// ---------------------------------------------------------------------------
// Small-table path, v2.  Same LDS layout and slab flush as ingest_lds_kernel;
// the span loop is rebuilt for latency tolerance at 16 waves per CU:
//   * kTilesInFlight (2) tiles of kSpansPerLane (2) spans per lane in flight
//     per wave (a register ring): a tile is re-filled right after it is
//     compacted, so every wave keeps loads outstanding while it computes;
//   * the key lookup reads the key's two 4-slot buckets from the LDS mirror
//     (4 x 16-B reads, fixed cost, no probe loop); only keys outside their two
//     buckets (a few % of a 0.7-load table, none at all after the first
//     launch for C2) take the wave-uniform cold path;
//   * HLL register reads are issued one step ahead of their compare, so the
//     wait for them is a counted vmcnt that leaves two tiles in flight;
//   * event statistics are per-wave ballot counts (scalar registers).
// LDS: lkeys[cap] u64 | lsum[cap] u64 | lcnt[cap][nw] u32 | hq[kHllQueue] u64 |
//      hq_n (16 B) | bins[kBins]
// Wave-cooperative find-or-insert of ONE (wave-uniform) key: the 64 lanes
// test 64 consecutive positions of its probe sequence at once, first in the
// LDS mirror, then in the HBM table (where the first empty position is
// claimed by CAS).  No divergent loop, so no per-lane exec-mask nesting.
// Must be called with all lanes active; returns the slot (uniform) or
// kNotFound when the table is full.
__device__ __forceinline__ uint32_t wave_find_insert(unsigned long long *lkeys, uint64_t k,
                                                     uint32_t log2cap) {
  SA_CONST const IngestParams &Q = cold_params();
  const uint32_t lane = threadIdx.x & 63;
  const ProbeSeq pr = probe_seq(k, log2cap);
  const uint32_t maxp = Q.max_probe;
  for (uint32_t i0 = 0; i0 < maxp; i0 += 64) {  // LDS mirror
    const uint32_t pos = i0 + lane;
    const uint32_t sl = seq_slot(pr, pos < maxp ? pos : maxp - 1);
    const unsigned long long v = lkeys[sl];
    const uint64_t mh = __ballot(v == k), me = __ballot(v == 0);
    if (mh | me) {
      if (mh && (!me || __builtin_ctzll(mh) < __builtin_ctzll(me)))
        return (uint32_t)__builtin_amdgcn_readlane((int)sl, __builtin_ctzll(mh));
      break;
    }
  }
  SA_GLOBAL unsigned long long *gk = gbl(Q.gkeys);
  for (uint32_t i0 = 0; i0 < maxp;) {  // HBM table
    const uint32_t pos = i0 + lane;
    const uint32_t sl = seq_slot(pr, pos < maxp ? pos : maxp - 1);
    const unsigned long long v = __hip_atomic_load(&gk[sl], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t mh = __ballot(v == k), me = __ballot(v == 0 && pos < maxp);
    if (!(mh | me)) {
      i0 += 64;
      continue;
    }
    const int first = __builtin_ctzll(mh | me);
    const uint32_t fsl = (uint32_t)__builtin_amdgcn_readlane((int)sl, first);
    if ((mh >> first) & 1) {
      lkeys[fsl] = k;
      return fsl;
    }
    unsigned long long prev = 0;
    if ((int)lane == first) {
      unsigned long long expect = 0;
      __hip_atomic_compare_exchange_strong(&gk[fsl], &expect, (unsigned long long)k,
                                           __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
      prev = expect;
    }
    const uint32_t plo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)prev, first);
    const uint32_t phi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(prev >> 32), first);
    const uint64_t pv = ((uint64_t)phi << 32) | plo;
    if (pv == 0 || pv == k) {
      lkeys[fsl] = k;
      return fsl;
    }
    i0 += (uint32_t)first;  // lost the race for that slot: re-read from it
  }
  return kNotFound;
}

// Resolves the lanes with `need` one distinct key at a time (lanes sharing a
// key are resolved together); call with all lanes active.
__device__ __forceinline__ void cold_lookup_wave(unsigned long long *lkeys, bool need, uint64_t key,
                                                 uint32_t log2cap, uint32_t &found) {
  uint64_t m = __ballot(need);
  while (m) {
    const int l = __builtin_ctzll(m);
    const uint32_t klo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)key, l);
    const uint32_t khi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(key >> 32), l);
    const uint64_t k = ((uint64_t)khi << 32) | klo;
    const uint32_t f = wave_find_insert(lkeys, k, log2cap);
    const bool same = need && key == k;
    found = same ? f : found;
    m &= ~__ballot(same);
  }
}

// Adds one ERROR span of (window slot, key slot) key `ek` (< 65535) to the
// workgroup's LDS table: 256 aligned groups of 4 entries {(ek + 1) << 16 |
// count}; false when the key's group is taken by other keys (the caller then
// falls back to a global atomic).  The common case -- the key already in its
// group -- is one ds_read_b128, four compares and one ds_add; the claim loop
// runs once per key per workgroup.  (A linear 4-probe loop with a CAS per
// probe compiled to ~100 mostly scalar instructions per wave step: 2 % of
// spans are ERROR, so nearly every 128-span wave step has one.)
__device__ __forceinline__ bool lds_err_add(uint32_t *etab, uint32_t ek) {
  const uint32_t tag = (ek + 1) << 16;
  uint32_t *grp = etab + ((ek * 0x9E3779B1u) >> (32 - 8)) * 4;  // kErrTab = 1024
  const uint4 v = *reinterpret_cast<const uint4 *>(grp);
  const int at = (v.x & 0xFFFF0000u) == tag   ? 0
                 : (v.y & 0xFFFF0000u) == tag ? 1
                 : (v.z & 0xFFFF0000u) == tag ? 2
                 : (v.w & 0xFFFF0000u) == tag ? 3
                                              : -1;
  if (__builtin_expect(at >= 0, 1)) {
    atomicAdd(grp + at, 1u);
    return true;
  }
  for (int q = 0; q < 4; ++q) {
    uint32_t w = grp[q];
    if (w == 0) {
      w = atomicCAS(grp + q, 0u, tag | 1u);
      if (w == 0) return true;
    }
    if ((w & 0xFFFF0000u) == tag) {
      atomicAdd(grp + q, 1u);
      return true;
    }
  }
  return false;
}

// LC / NWC / PC: table log2 capacity, counter words per slot and HLL precision
// fixed at compile time for the common geometry (0 = read from P).
// Tiles are read with the nt cache policy (streamed once), HLL registers with
// plain global loads.
// Inside the workgroup's range, waves claim chunks of kTilesInFlight
// wave-tiles from an LDS counter instead of owning a fixed slice of every
// workgroup tile, so waves the memory arbiter serves late simply take fewer
// chunks and all 16 finish together (the fixed split left the 4 youngest waves
// of every workgroup streaming alone for the last ~25% of the launch).  A
// grid-wide counter in HBM was tried first: its returning atomic put a
// vmcnt(0) at the top of every round and ran 3.4x slower.
// LEAN: every wave issues its key-table loads before any wave issues tile
// loads (a workgroup barrier between them), so the LDS setup does not wait
// behind the other waves' first tiles; rare events in LDS counters and, with a
// compile-time geometry, the two-phase epilogue (v2_epilogue); the span hash
// on 32-bit halves (xxh64_16_h), rho / register index without 64-bit shifts,
// the register row offset by a 24-bit multiply, and the wave-level dedup of
// the hot series' counter adds.
// EXPO: exponential-histogram engines (spanagg_expo.hip does the buckets).
// The RED update becomes per-slot LDS header partials -- count, zero count,
// ns sum, max of ~d and max d over positive durations (XHdr) -- in the space
// of lsum + lcnt (nw = 6: 32 B per slot), written to the workgroup's header
// slab at the end; every span's key slot goes to P.slot_of for the
// bucket-counting pass.
// A wave's claim of the next chunk from an LDS counter kept in units of
// 1/64 chunk.  Every lane adds the same 1 (no branch: a divergent claim made
// the compiler wait for it at the join), so the atomic optimizer issues one
// ds_add_rtn of popcount(exec) = 64 and hands the lanes base + rank; the first
// lane's base / 64 is the claim.  (A lane-varying addend -- 1 on lane 0, 0
// elsewhere -- compiled to a 64-iteration readlane/writelane scan loop per
// claim: ~140 scalar and ~30 vector instructions per span-lane of the C2 loop.)
// Requires a full wave at the call, which the claim loops have.
__device__ __forceinline__ uint32_t wave_claim(uint32_t *ctr) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)atomicAdd(ctr, 1u)) >> 6;
}

constexpr int kSpansPerLane = 2;   // one 16-B load per u64 column per lane and tile
constexpr int kTilesInFlight = 2;  // a wave's register ring of tiles (= the tiles of one claim)

// ---------------------------------------------------------------------------
// The phases of ingest_v2_kernel's step, per span unless said otherwise.

// Step 4: the key's two candidate 4-slot buckets in the LDS mirror (4 x 16-B
// reads, fixed cost, no probe loop): its slot, or kNotFound.
__device__ __forceinline__ uint32_t two_bucket_lookup(const unsigned long long *lkeys, unsigned long long k,
                                                      uint32_t log2cap) {
  const ProbeSeq pr = probe_seq(k, log2cap);
  const ulonglong2 *b1 = reinterpret_cast<const ulonglong2 *>(lkeys + pr.b1 * 4);
  const ulonglong2 *b2 = reinterpret_cast<const ulonglong2 *>(lkeys + pr.b2 * 4);
  const ulonglong2 q1a = b1[0], q1b = b1[1], q2a = b2[0], q2b = b2[1];
  uint32_t f = kNotFound;
  f = q2b.y == k ? pr.b2 * 4 + 3 : f;
  f = q2b.x == k ? pr.b2 * 4 + 2 : f;
  f = q2a.y == k ? pr.b2 * 4 + 1 : f;
  f = q2a.x == k ? pr.b2 * 4 + 0 : f;
  f = q1b.y == k ? pr.b1 * 4 + 3 : f;
  f = q1b.x == k ? pr.b1 * 4 + 2 : f;
  f = q1a.y == k ? pr.b1 * 4 + 1 : f;
  f = q1a.x == k ? pr.b1 * 4 + 0 : f;
  return f;
}

// Step 6, an ERROR span: the exact per-(window, slot) counter -- the
// workgroup's LDS table, else one no-return global atomic; a span without a
// slot updates the count-min cells directly.
__device__ __forceinline__ void error_add(uint32_t *etab, bool err_lds, uint32_t ws, uint32_t found, uint64_t key,
                                          uint32_t log2cap) {
  if (found == kNotFound) {
    cold_cms_add(ws, key);
  } else {
    const uint32_t ek = (ws << log2cap) | found;
    if (!(err_lds && lds_err_add(etab, ek)))
      atomicAdd(cold_params().errcnt + ((uint64_t)ws << log2cap) + found, 1ULL);
  }
}

// Step 7, the RED update of a span; the hot series' ns sum goes to the lane's
// register (hot_sum), the others' to LDS.  (The LEAN form is in the kernel.)
// Plain: LDS u16 bucket counter + u64 ns sum.
template <bool DIAG>
__device__ __forceinline__ void red_update_plain(const SmallLds &L, uint32_t nw, uint32_t cap, uint32_t diag,
                                                 uint32_t found, uint32_t b, uint64_t dur, uint32_t hot_slot,
                                                 unsigned long long &hot_sum) {
  if (found != kNotFound) {
    // diag 4096: spread the atomics over slots by lane (prices same-address
    // serialisation of hot keys; counts are wrong)
    const uint32_t fs = (DIAG && (diag & 4096u)) ? (found + (threadIdx.x & 63u) * 29u) & (cap - 1u) : found;
    atomicAdd(&L.lcnt[fs * nw + (b >> 1)], 1u << ((b & 1) * 16));
    if (found == hot_slot) hot_sum += dur;
    else atomicAdd(&L.lsum[fs], (unsigned long long)dur);
  }
}
// EXPO: per-slot LDS header partials -- count, zero count, ns sum, max of ~d
// and max d over positive durations (XHdr) -- in the space of lsum + lcnt.
struct XPartials {
  unsigned long long *minx, *max;
  uint32_t *cnt, *zero;
};
__device__ __forceinline__ XPartials expo_partials(const SmallLds &L, uint32_t cap) {
  uint32_t *const cnt = reinterpret_cast<uint32_t *>(L.lsum + 3 * cap);
  return {L.lsum + cap, L.lsum + 2 * cap, cnt, cnt + cap};
}
__device__ __forceinline__ void red_update_expo(const SmallLds &L, const XPartials &X, uint32_t f, unsigned long long d,
                                                uint32_t hot_slot, unsigned long long &hot_sum) {
  if (f != kNotFound) {
    atomicAdd(&X.cnt[f], 1u);
    if (f == hot_slot) hot_sum += d;
    else atomicAdd(&L.lsum[f], d);
    if (d == 0) {
      atomicAdd(&X.zero[f], 1u);
    } else {
      atomicMax(&X.minx[f], ~d);
      atomicMax(&X.max[f], d);
    }
  }
}
// The laboratory's SPANAGG_XIDX_OFF ablations of the EXPO index records
// (P.xidx 2: wrong buckets without the index computation; 3: also without the
// scale read); the product build has none.  A macro, so that the product's 0
// is folded before code generation (a function of P, folded after inlining,
// changed the EXPO instances' device code).  kLabBuild: whether the ablation
// option set (O::DIAG) may be instantiated at all.
#ifdef SPANAGG_AB
#define SA_XIDX_ABLATION(P) ((P).xidx >= 2 ? (P).xidx : 0u)
constexpr bool kLabBuild = true;
#else
#define SA_XIDX_ABLATION(P) 0u
constexpr bool kLabBuild = false;
#endif

// The prologue's LDS setup, up to (not including) its barrier, from the
// values its loads brought: the key table kv, the bin table bv, the HLL bounds
// lbw.  (The loads themselves, and EXPO's scale bytes, stay in the kernel: as
// functions they raised the generic EXPO instance's SGPR spills.)
template <uint32_t BLK>
__device__ __forceinline__ void lds_setup(const IngestParams &P, const SmallLds &L, uint32_t cap, uint32_t nw, bool lb_on,
                                          const ulonglong2 (&kv)[4], uint4 bv, uint32_t lbw) {
  const uint32_t per = (cap + 2 * BLK - 1) / (2 * BLK);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t i = 2 * (threadIdx.x + u * BLK);
    if (u < (int)per && i < cap) {
      reinterpret_cast<ulonglong2 *>(L.lkeys)[i / 2] = kv[u];
      reinterpret_cast<ulonglong2 *>(L.lsum)[i / 2] = make_ulonglong2(0, 0);
    }
  }
  if (threadIdx.x < kBins * 2) reinterpret_cast<uint4 *>(L.lbins)[threadIdx.x] = bv;
  for (uint32_t i = threadIdx.x * 4; i < cap * nw; i += BLK * 4)
    *reinterpret_cast<uint4 *>(L.lcnt + i) = make_uint4(0, 0, 0, 0);
  if (threadIdx.x == 0) {
    L.hq_n[0] = 0;
    // the next unclaimed chunk of this workgroup's range, x 64 (see wave_claim)
    L.hq_n[1] = (2u * (BLK / 64)) << 6;
    L.hq_n[2] = 0;  // HLL updates the lower-bound filter skipped (summed over the waves)
  }
  if (threadIdx.x < 4) L.lstat[threadIdx.x] = 0;
  for (uint32_t i = threadIdx.x; i < kErrTab; i += BLK) L.etab[i] = 0;
  // (filter off: the first bound word stays 0, and every span's sub-block
  // index is 0 or 1 below, so no rho can be at or below it)
  if (threadIdx.x * 4 < (lb_on ? P.lb_n : 4u)) reinterpret_cast<uint32_t *>(L.llb)[threadIdx.x] = lbw;
}

// The event counts at the kernel's end (after the epilogue's barrier, so the
// LDS counts are final).  LEAN's LDS counters: one global add per count.
__device__ __forceinline__ void flush_lds_stats(const uint32_t *lstat) {
  if (threadIdx.x < 4 && lstat[threadIdx.x]) {
    constexpr uint32_t kIdx[4] = {kStatZeroKey, kStatInvalidService, kStatWindowOOR, kStatDropped};
    atomicAdd(&cold_params().stats[kIdx[threadIdx.x]], (unsigned long long)lstat[threadIdx.x]);
  }
}
// The filtered HLL updates (hq_n[2]), to a slot per workgroup: thousands of
// same-address atomics at the end of every launch would serialise its tail.
__device__ __forceinline__ void flush_filtered(const uint32_t *hq_n) {
  if (threadIdx.x == 0 && hq_n[2])
    atomicAdd(&cold_params().hll_filt[blockIdx.x & (kFiltSlots - 1)], (unsigned long long)hq_n[2]);
}
// The plain form's wave-uniform counts: one add per wave and count.
__device__ __forceinline__ void flush_wave_stats(uint32_t n_zero, uint32_t n_badsvc, uint32_t n_oor, uint32_t n_drop) {
  if ((threadIdx.x & 63) == 0) {
    unsigned long long *const stats = cold_params().stats;
    if (n_zero) atomicAdd(&stats[kStatZeroKey], (unsigned long long)n_zero);
    if (n_badsvc) atomicAdd(&stats[kStatInvalidService], (unsigned long long)n_badsvc);
    if (n_oor) atomicAdd(&stats[kStatWindowOOR], (unsigned long long)n_oor);
    if (n_drop) atomicAdd(&stats[kStatDropped], (unsigned long long)n_drop);
  }
}

// The kernel's epilogue (after the loop's workgroup barrier) in its three
// forms: EXPO, the compile-time geometries' prefetched one (v2_epi_pre +
// v2_epilogue above) and the generic one.
// EXPO: this workgroup's header partials -> its slab, every slot (untouched
// ones as zeros: the reduce pass reads the slab and leaves it as it is, no
// zeroing stores behind its reads); the ERROR counts; the HLL raises and bound.
template <uint32_t B, uint32_t Q>
__device__ __forceinline__ void epilogue_expo(const IngestParams &P, const SmallLds &L, const XPartials &X, uint32_t cap,
                                              uint32_t log2cap, bool err_lds, const uint32_t *hqv, uint32_t nq,
                                              const uint4 (&lv)[4]) {
  XHdr *xs = P.xslab + (uint64_t)blockIdx.x * cap;
  for (uint32_t sl = threadIdx.x; sl < cap; sl += B) xs[sl] = XHdr{X.cnt[sl], X.zero[sl], L.lsum[sl], X.minx[sl], X.max[sl]};
  errtab_to_slab<B, true>(P, L.etab, err_lds, log2cap);
  epi_raise_and_bound<B, Q>(cold_params(), L.hq, hqv, nq, lv);
}
// Generic: the slab flush of ingest_lds_kernel, the ERROR counts, the queued
// HLL raises and a refresh of the bounds, all read after the barrier.
template <uint32_t B>
__device__ __forceinline__ void epilogue_generic(const IngestParams &P, const SmallLds &L, uint32_t cap, uint32_t nw,
                                                 uint32_t log2cap, bool err_lds, uint32_t nq) {
  flush_lds(P, cap, nw, L.lsum, L.lcnt);
  errtab_to_slab<B, false>(P, L.etab, err_lds, log2cap);
  for (uint32_t i = threadIdx.x; i < nq; i += B) hll_raise(P.hll + L.hq[i].x, L.hq[i].y);
  hll_lb_refresh(P, threadIdx.x >> 6, B / 64);
}

//
// The kernel's template: its geometry (LC = log2 slots, NWC = counter words
// per slot, PC = HLL precision; 0 = read from P), EXPO, the block size and an
// option set O (LEAN above; DIAG: honour the SA_DIAG_* ablation bits).  The
// product's two option sets are V2Lean (the default table, the 512-thread
// generic kernel and every EXPO engine) and V2Plain (the 1,024-thread generic
// kernel); the laboratory's ablation set V2Diag is defined in
// lab/small_lab.inc, which only the laboratory build compiles.
struct V2Plain {
  static constexpr bool LEAN = false, DIAG = false;
};
struct V2Lean : V2Plain {
  static constexpr bool LEAN = true;
};
template <int LC, int NWC, int PC, bool EXPO, uint32_t BLK, typename O>
__global__ __launch_bounds__(BLK) void ingest_v2_kernel(IngestParams P) {
  constexpr int S = kSpansPerLane, NBUF = kTilesInFlight, AUX = 2;  // (AUX 2: nt tile loads)
  constexpr bool LEAN = O::LEAN, DIAG = O::DIAG;
  static_assert(kLabBuild || !DIAG, "laboratory switch: libspanagg_ab.so only");
  static_assert(BLK % 64 == 0 && kErrTab % BLK == 0 && kHllQueue % BLK == 0 && BLK * 4 >= kLbMaxSub, "block size");
  static_assert(S == 2, "EXPO stores a lane's two spans as one vector");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  if (P.dbg && threadIdx.x == 0) P.dbg[blockIdx.x * kDbgPerWg + 0] = __builtin_amdgcn_s_memrealtime();
  const uint32_t log2cap = LC ? (uint32_t)LC : P.log2cap;
  const uint32_t cap = 1u << log2cap;
  const uint32_t nw = EXPO ? (uint32_t)kExpoWords : NWC ? (uint32_t)NWC : (P.nbk + 1) >> 1;
  const uint32_t hp = PC ? (uint32_t)PC : P.p;
  const uint32_t diag = DIAG ? P.diag : 0u;
  const SmallLds L = small_lds_carve(smem, cap, nw, EXPO);
  unsigned long long *const lkeys = L.lkeys, *const lsum = L.lsum;
  uint32_t *const lcnt = L.lcnt, *const hq_n = L.hq_n, *const lstat = L.lstat, *const etab = L.etab;
  uint2 *const hq = L.hq;
  BinEntry *const lbins = L.lbins;
  uint8_t *const llb = L.llb;
  int8_t *const lsc = L.lsc;
  // the compile-time-geometry epilogue (v2_epilogue) raises from the word each
  // span saw: the queue region holds kQcap (hoff, rho) pairs, then their words
  constexpr bool kObs = (LC != 0 && NWC != 0 && LEAN) || EXPO;
  constexpr uint32_t kQcap = kObs ? kHllQueue / 2 : kHllQueue;
  static_assert(!kObs || kQcap * 12 <= kHllQueue * 8, "queue region");
  uint32_t *hqv = reinterpret_cast<uint32_t *>(hq + kQcap);
  const bool err_lds = P.errslab != nullptr;
  const bool lb_on = P.lb_n != 0 && !(diag & 2u);
  const XPartials X = expo_partials(L, cap);  // EXPO header partials (zeroed with lsum / lcnt)

  uint64_t lo, hi;
  wg_range_p(P, lo, hi);
  const uint32_t len = (uint32_t)(hi - lo);
  // a step covers one wave tile (64 * S spans, lane_off by lane) and a claim
  // is NBUF consecutive wave tiles
  constexpr uint32_t tile = 64 * S;
  constexpr uint32_t chunk = NBUF * tile;
  const uint32_t lane_off = (threadIdx.x & 63u) * S;
  constexpr uint32_t kWaves = BLK / 64;
  const uint32_t n_chunks = (len + chunk - 1) / chunk;
  // wave-uniform by construction; readfirstlane keeps it (and every tile
  // base derived from it) in SGPRs for the buffer descriptors
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the first two chunks of every wave are fixed; claims continue after them
  uint32_t c0 = wave, c1 = wave + kWaves;
  auto tstart = [&](uint32_t c, int b) -> uint32_t {  // step b's first span in chunk c, relative to lo
    return c * chunk + (uint32_t)b * tile;
  };
  auto tremain = [&](uint32_t t) -> uint32_t { return len > t ? len - t : 0u; };

  // Prologue: key-table loads (16 B per lane, <= 4 per lane for cap <= 8192)
  // and the bin table first, then the first NBUF tiles; the LDS setup
  // (lds_setup) then waits only for the key-table loads (vmcnt counts in
  // issue order).  (The loads are inline: as a function returning their values
  // they raised the generic EXPO instance's SGPR spills, 80 -> 82 or 84.)
  ulonglong2 kv[4];
  const uint32_t per = (cap + 2 * BLK - 1) / (2 * BLK);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const uint32_t i = 2 * (threadIdx.x + u * BLK);
    kv[u] = (u < (int)per && i < cap) ? *reinterpret_cast<const ulonglong2 *>(P.gkeys + i)
                                      : make_ulonglong2(0, 0);
  }
  uint4 bv = make_uint4(0, 0, 0, 0);
  if (!EXPO && threadIdx.x < kBins * 2) bv = reinterpret_cast<const uint4 *>(P.bintab)[threadIdx.x];  // (EXPO: no buckets)
  // EXPO with index records: the slots' scales (cap <= 2,048 bytes: a 16-bit
  // pair per thread), issued with the key table so the LDS setup waits for
  // them and not for the first tiles
  uint32_t xsc = 0;
  if constexpr (EXPO)
    if (P.xidx && SA_XIDX_ABLATION(P) != 3 && 2 * threadIdx.x < cap) xsc = *reinterpret_cast<const uint16_t *>(P.xscale + 2 * threadIdx.x);
  uint32_t lbw = 0;
  if (lb_on && threadIdx.x * 4 < P.lb_n) lbw = *reinterpret_cast<const uint32_t *>(P.hll_lb + threadIdx.x * 4);
  if constexpr (LEAN) {
    // no wait here (gfx950 barriers do not drain vmcnt): only the issue order
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  }
  // Issue order = the steady state's (tile, then S HLL reads, per step), so
  // the loop header's vmcnt accounting is the same from both predecessors;
  // the prologue's HLL reads seed `pend` (rho 0: never raised).
  SpanTile<S> buf[NBUF];
  Pending<S> pend;
#pragma unroll
  for (int b = 0; b < NBUF; ++b) {
    const uint32_t t = tstart(c0, b);
    load_tile_at<S, AUX>(P, (diag & 16u) ? t % (4 * tile) : lo + t, tremain(t), lane_off, buf[b]);
    if (b == NBUF - 1) {
      uint32_t z;  // a VGPR zero: keeps these vector loads (a uniform address would be s_load)
      asm volatile("v_mov_b32 %0, 0" : "=v"(z));
#pragma unroll
      for (int j = 0; j < S; ++j) pend.hv[j] = *reinterpret_cast<const uint32_t *>(P.hll + z);
    }
  }
  lds_setup<BLK>(P, L, cap, nw, lb_on, kv, bv, lbw);
  if constexpr (EXPO)
    if (P.xidx && SA_XIDX_ABLATION(P) != 3 && 2 * threadIdx.x < cap) *reinterpret_cast<uint16_t *>(lsc + 2 * threadIdx.x) = (uint16_t)xsc;
  __syncthreads();
  if (P.dbg && threadIdx.x == 0) P.dbg[blockIdx.x * kDbgPerWg + 1] = __builtin_amdgcn_s_memrealtime();

  // diagnostic build: per-wave cycle sums of the step's segments (s_memtime;
  // the stamp's lgkmcnt(0) serialises LDS, so read shares, not lengths)
  uint64_t seg[6] = {0, 0, 0, 0, 0, 0}, t_prev = 0;
  auto stamp = [&](int i) {
    if (DIAG && P.dbg) {
      __builtin_amdgcn_sched_barrier(0);
      uint64_t t;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      __builtin_amdgcn_sched_barrier(0);
      if (i >= 0) seg[i] += t - t_prev;
      t_prev = t;
    }
  };
  stamp(-1);
  // the bound's shift as a VGPR operand (31 with the filter off): a loop-long
  // scalar here was one of the kernel's SGPR spills, read back by a
  // v_readlane on every span
  const uint32_t lbs_v = copy_u32(lb_on ? P.lb_shift : 31u);
  const uint32_t wmask_v = copy_u32(P.win_mask);  // (likewise the ring mask of every span's window slot)
  constexpr uint32_t kHotUnset = 0xFFFFFFFEu;
  uint32_t hot_slot = kHotUnset;  // wave-uniform (see step 5b)
  unsigned long long hot_sum = 0;
  // wave-uniform event counts (scalar registers)
  uint32_t n_zero = 0, n_badsvc = 0, n_oor = 0, n_drop = 0;
  uint32_t n_filt = 0;  // per lane: HLL updates the lower-bound filter skipped
#pragma unroll
  for (int j = 0; j < S; ++j) pend.hoff[j] = pend.rho[j] = 0;

  // HLL compare of the previous step's reads; registers that grow are queued
  // in LDS and raised after the loop (no returning global atomic in the loop).
  auto hll_settle = [&](const Pending<S> &q) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
      // hv: the aligned u32 word holding the register (a u8 load would be
      // zero-extended by a v_and at the loop-carried copy, which waits for it)
      if (((q.hv[j] >> ((q.hoff[j] & 3u) * 8)) & 0xFFu) < q.rho[j]) {
        const uint32_t slot = atomicAdd(hq_n, 1u);
        if (slot < kQcap) {
          hq[slot] = make_uint2(q.hoff[j], q.rho[j]);
          if constexpr (kObs) hqv[slot] = q.hv[j];
        } else {
          cold_hll_raise(q.hoff[j], q.rho[j]);
        }
      }
    }
  };

  // step: consume the landed tile T (first span toff) and re-fill its
  // registers with the tile at pf (relative to lo)
  auto step = [&](SpanTile<S> &T, uint32_t toff, uint32_t pf) {
    // 1. compact the landed tile (its registers are re-filled in step 3)
    uint64_t key[S], dur[S];
    uint32_t bkt[S], ws[S], hoff[S], rho[S];
    bool err[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      const bool valid = lane_off + toff + (uint32_t)j < len;
      // 0 past the range (buffer bounds check).  An explicit copy: the key is
      // used after the tile registers are re-filled, and sharing them would
      // make the allocator rotate the tile ring through copies that wait.
      key[j] = copy_u64(T.key[j]);
      if (!(diag & 128u) && !LEAN) n_zero += wave_count(valid && key[j] == 0);
      dur[j] = T.e[j] > T.s[j] ? T.e[j] - T.s[j] : 0;
      bkt[j] = EXPO ? 0u : (diag & 32u) ? (uint32_t)dur[j] & 15u : bucket_lds<1>(dur[j], lbins, P);
      const uint32_t meta = copy_u32(T.meta[j]);  // see key
      const uint32_t svc = meta & 0xFFFFu;
      const bool svc_ok = svc < P.n_services;
      ws[j] = (diag & 64u) ? (uint32_t)(T.e[j] >> 34) & 7u : LEAN ? window_slot_lean(P, T.e[j], wmask_v) : window_slot(P, T.e[j]);
      const bool win_ok = ws[j] != 0xFFFFFFFFu;
      if (!(diag & 128u)) {
        if constexpr (LEAN) {
          // rare events: LDS counters (no wave-uniform accumulators held in
          // scalar registers across the loop)
          const uint32_t ev = (valid && key[j] == 0 ? 1u : 0u) | (valid && !svc_ok ? 2u : 0u) |
                              (valid && svc_ok && !win_ok ? 4u : 0u);
          if (__builtin_expect(ev != 0, 0)) {
            if (ev & 1u) atomicAdd(&lstat[0], 1u);
            if (ev & 2u) atomicAdd(&lstat[1], 1u);
            if (ev & 4u) atomicAdd(&lstat[2], 1u);
          }
        } else {
          n_badsvc += wave_count(valid && !svc_ok);
          n_oor += wave_count(valid && svc_ok && !win_ok);
        }
      }
      const bool sk = valid && svc_ok && win_ok;
      err[j] = sk && ((meta >> 19) & 3u) == 2u && !(diag & 4u);
      rho[j] = 0;
      hoff[j] = 0;
      if (!(diag & 2u)) {
        // rho, register index and row in the LEAN and the plain form (inline:
        // as two functions returning the three values they cost every instance
        // but the default one a VGPR and three of them SGPR spills)
        uint32_t r, idx, row;
        if constexpr (LEAN) {
          const H64 x = xxh64_16_h(T.a[j], T.b[j]);
          const uint32_t yh = __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - hp);  // (x << hp) >> 32
          const uint32_t yl = (x.lo << hp) | (1u << (hp - 1));
          r = (uint32_t)__clzll((long long)(((uint64_t)yh << 32) | yl)) + 1;  // 2 x v_ffbh, no 64-bit shift
          idx = x.hi >> (32 - hp);
          // ws < 2^12, n_services <= 2^16: a 24-bit multiply-add (LLVM picks
          // the quarter-rate v_mad_u64_u32 for the plain expression)
          asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(ws[j]), "s"(P.n_services), "v"(svc));
        } else {
          // diag 16384: one 64-bit multiply instead of xxh64 (prices the hash's VALU)
          const uint64_t x = (DIAG && (diag & 16384u)) ? (T.a[j] ^ T.b[j]) * XP1 : xxh64_16(T.a[j], T.b[j]);
          r = (uint32_t)__clzll((long long)((x << hp) | (1ULL << (hp - 1)))) + 1;
          idx = (uint32_t)(x >> (64 - hp));
          row = ws[j] * P.n_services + svc;
        }
        const uint32_t ho = sk ? (row << hp) + idx : 0u;
        // a rho at or below the register sub-block's lower bound cannot raise it
        const bool up = sk && !(r <= llb[ho >> lbs_v]);
        n_filt += (sk && !up) ? 1u : 0u;
        rho[j] = up ? r : 0u;
        hoff[j] = up ? ho : 0u;
      }
    }
    stamp(0);
    // 2. this step's HLL register reads (unconditional: offset 0 when unused)
    uint32_t hv[S];
#pragma unroll
    for (int j = 0; j < S; ++j) {
      if (DIAG && (diag & 512u)) {  // diag: blind byte store instead of the read
        P.hll[hoff[j]] = (uint8_t)rho[j];
        hv[j] = 0xFFFFFFFFu;
      } else if (DIAG && (diag & 1024u)) {  // diag: no read at all
        hv[j] = 0xFFFFFFFFu;
      } else {
        hv[j] = *reinterpret_cast<const uint32_t *>(P.hll + (hoff[j] & ~3u));
      }
    }
    // 3. re-fill the tile registers with the tile NBUF steps ahead
    __builtin_amdgcn_sched_barrier(0);
    load_tile_at<S, AUX>(P, (diag & 16u) ? pf % (4 * tile) : lo + pf, tremain(pf), lane_off, T);
    __builtin_amdgcn_sched_barrier(0);
    stamp(1);
    // 4. key lookup: the two candidate buckets in the LDS mirror
    uint32_t found[S];
    if (!(diag & 1u)) {
      bool need[S];
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const unsigned long long k = key[j];
        const uint32_t f = two_bucket_lookup(lkeys, k, log2cap);
        found[j] = k != 0 ? f : kNotFound;
        need[j] = k != 0 && f == kNotFound;
      }
      // 5. cold path (wave-uniform): keys outside their two buckets or not yet
      //    in this workgroup's mirror
#pragma unroll
      for (int j = 0; j < S; ++j) {
        if (__builtin_expect(__ballot(need[j]) != 0, 0)) {
          cold_lookup_wave(lkeys, need[j], key[j], log2cap, found[j]);
          if constexpr (LEAN) {
            if (need[j] && found[j] == kNotFound) atomicAdd(&lstat[3], 1u);
          } else {
            n_drop += wave_count(need[j] && found[j] == kNotFound);
          }
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j) {
        found[j] = kNotFound;
        n_drop += wave_count(((key[j] ^ dur[j] ^ bkt[j]) & 0xFFFFFFFFFFFFULL) == 0x123456789ABCULL);
      }
    }
    stamp(2);
    // wave-level key dedup (first step only): the wave's hot series is the
    // most common slot among four candidate lanes (ballot); its ns sum then
    // accumulates in a lane register instead of the LDS atomic that every lane
    // of that series would otherwise serialise on (summed once at the end)
    // (inline: as a function it inverted two branches of the timed instances)
    if (hot_slot == kHotUnset) {
      uint32_t best = kNotFound, nbest = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t cand = (uint32_t)__builtin_amdgcn_readlane((int)found[0], c * 16);
        const uint32_t n = wave_count(found[0] == cand);
        if (cand != kNotFound && n > nbest) {
          best = cand;
          nbest = n;
        }
      }
      hot_slot = best;
    }
    // 6. ERROR spans
#pragma unroll
    for (int j = 0; j < S; ++j)
      if (err[j]) error_add(etab, err_lds, ws[j], found[j], key[j], log2cap);
    // 7. RED update, in one of its three forms
    if constexpr (EXPO) {
      // + the span's slot, or its index record (the bucket index at the
      // slot's starting scale), or the span record, for the counting pass.
      // (Inline: as functions the index record and the two stores changed the
      // EXPO instances' registers and spills.)
      uint32_t xw[S] = {};
#pragma unroll
      for (int j = 0; j < S; ++j) {
        red_update_expo(L, X, found[j], dur[j], hot_slot, hot_sum);
        const uint32_t f = found[j];
        if (!P.span_rec) {
          uint32_t w = f;
          if (P.xidx) {
            // (branch-free but for the rare long-duration store: every lane
            // computes the index, the record is picked by selects)
            const unsigned long long d = dur[j];
            const bool nf = f == kNotFound;
            const uint32_t fs = nf ? 0u : f;
            const int32_t sc = SA_XIDX_ABLATION(P) == 3 ? 0 : lsc[fs];
            int32_t ix = 0;
            bool ok;
            if (SA_XIDX_ABLATION(P) >= 2) ok = true, ix = (int32_t)(d & 7u);  // (wrong buckets)
            else ok = expo_index_fast(d ? d : 1u, P.l2d_q24, sc, ix) && ix >= kIxMin && ix <= kIxMax;
            w = nf ? kSpanRecNoSlot << kIxSlotShift
                   : d == 0 ? (f << kIxSlotShift | kIxZero)
                            : ok ? ixrec_of(f, sc, ix) : (f << kIxSlotShift | kIxLong);
            if (!nf && d != 0 && !ok && lane_off + toff + (uint32_t)j < len) P.span_long[lo + toff + lane_off + j] = d;
          }
          xw[j] = w;
        }
      }
      // the lane's slots / index records: one 8-B store for its two spans
      // (lo, toff and lane_off are even)
      if (!P.span_rec) {
        const uint32_t i0 = toff + lane_off;
        uint32_t *wp = P.slot_of + lo + i0;
        if (i0 + 1 < len) *reinterpret_cast<uint2 *>(wp) = make_uint2(xw[0], xw[1]);
        else if (i0 < len) wp[0] = xw[0];
      }
      // the lane's span records: one 16-B store for its two spans (two 8-B
      // stores per lane cost the kernel ~24 us per 10 M spans)
      if (P.span_rec) {
        const uint32_t i0 = toff + lane_off;
        unsigned long long *rp = P.span_rec + lo + i0;
        if (i0 + 1 < len) {
          *reinterpret_cast<ulonglong2 *>(rp) =
              make_ulonglong2(span_rec_of(found[0], dur[0]), span_rec_of(found[1], dur[1]));
        } else if (i0 < len) {
          rp[0] = span_rec_of(found[0], dur[0]);
        }
        // (durations past the record's field, 52 days or more: in full beside it)
#pragma unroll
        for (int j = 0; j < S; ++j)
          if (dur[j] >= kSpanRecDurMask && i0 + (uint32_t)j < len) P.span_long[lo + i0 + j] = dur[j];
      }
    } else if constexpr (LEAN) {
      // LDS u16 bucket counter + u64 ns sum with wave-level key dedup of the
      // counter adds -- the lanes that hold the same (slot, bucket) as the
      // wave's first lane of its hot series (a ballot on the readlane'd key)
      // make one LDS add of their count, from the first of them; the other
      // lanes add their own span.  (Inline: every function form tried changed
      // ~870 lines of the default instance's loop.)
      const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
      for (int j = 0; j < S; ++j) {
        const uint32_t key = (found[j] << 6) | bkt[j];  // found < 2^11 or kNotFound, bucket < 64
        const uint64_t hm = __ballot(found[j] == hot_slot && found[j] != kNotFound);
        uint32_t lead = 64u, ndup = 0u, kk = 0xFFFFFFFFu;
        if (hm) {  // wave-uniform
          lead = (uint32_t)__builtin_ctzll(hm);
          kk = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)lead);
          ndup = (uint32_t)__popcll(__ballot(key == kk));
        }
        const bool dup = key == kk;
        if (found[j] != kNotFound && (!dup || lane == lead)) {
          const uint32_t b = bkt[j];
          atomicAdd(&lcnt[found[j] * nw + (b >> 1)], (dup ? ndup : 1u) << ((b & 1) * 16));
        }
        if (found[j] == hot_slot) hot_sum += dur[j];
        else if (found[j] != kNotFound) atomicAdd(&lsum[found[j]], (unsigned long long)dur[j]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < S; ++j)
        red_update_plain<DIAG>(L, nw, cap, diag, found[j], bkt[j], dur[j], hot_slot, hot_sum);
    }
    stamp(3);
    // 8. settle the previous step's HLL reads, keep this step's for the next
    hll_settle(pend);
#pragma unroll
    for (int j = 0; j < S; ++j) {
      pend.hoff[j] = hoff[j];
      pend.rho[j] = rho[j];
      pend.hv[j] = hv[j];
    }
    stamp(4);
  };

  // Whole rounds of NBUF steps (a step past the range sees only zero-filled
  // lanes and does nothing): no exit between the steps of a round, so the
  // register allocator keeps each in-flight tile in one set of registers
  // across the back-edge instead of copying it (a copy waits for the loads).
  // c0: this round's chunk (its tiles are in buf), c1: the next round's
  // (prefetched during this round), c2: claimed now for the round after.
  // The claim returns while the round runs; its result is read at the end.
  while (c0 < n_chunks) {
    const uint32_t c2 = wave_claim(&hq_n[1]);
#pragma unroll
    for (int b = 0; b < NBUF; ++b) step(buf[b], tstart(c0, b), tstart(c1, b));
    c0 = c1;
    c1 = c2;
  }
  hll_settle(pend);
  if (hot_slot < cap) {  // the hot series' ns sum: one add per wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
      hot_sum += (unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)hot_sum, o, 64) |
                 ((unsigned long long)(uint32_t)__shfl_xor((int)(uint32_t)(hot_sum >> 32), o, 64) << 32);
    if ((threadIdx.x & 63u) == 0 && hot_sum) atomicAdd(&lsum[hot_slot], hot_sum);
  }
  // one LDS add per wave; one global add per workgroup after the epilogue
  n_filt = wave_sum(n_filt);
  if ((threadIdx.x & 63) == 0 && n_filt) atomicAdd(&hq_n[2], n_filt);
  // (parameters used only after the loop are read through the laundered
  // kernarg pointer, so they do not hold SGPRs across it)
  unsigned long long *const dbg = cold_params().dbg;
  const uint64_t wave_loop_end = dbg ? __builtin_amdgcn_s_memrealtime() : 0;
  if (dbg && threadIdx.x == 0) dbg[blockIdx.x * kDbgPerWg + 2] = __builtin_amdgcn_s_memrealtime();
  // the two-phase epilogues' loads, before the barrier (v2_epi_pre)
  constexpr bool kSlabPre = LC != 0 && NWC != 0 && LEAN && !EXPO;
  constexpr uint32_t kCapC = 1u << (LC ? LC : 1);
  constexpr int kUpt = kSlabPre ? (int)(kCapC * NWC / 2 / BLK) : 1, kSpt = kSlabPre ? (int)(kCapC / 2 / BLK) : 1;
  EpiPre<kUpt, kSpt> epre;
  if constexpr (kSlabPre) {
    static_assert((kCapC * NWC / 2) % BLK == 0 && (kCapC / 2) % BLK == 0, "epilogue geometry");
    v2_epi_pre<kUpt, kSpt, BLK>(cold_params(), cap, nw, epre);
  } else if constexpr (EXPO) {
    hll_lb_pre<BLK>(cold_params(), epre.lv);
  }
  __syncthreads();
  const uint32_t nq = *hq_n < kQcap ? *hq_n : kQcap;
  if constexpr (EXPO) {
    epilogue_expo<BLK, kQcap>(P, L, X, cap, log2cap, err_lds, hqv, nq, epre.lv);
  } else if constexpr (kSlabPre) {
    v2_epilogue<kUpt, kSpt, BLK, kQcap>(cold_params(), cap, nw, log2cap, lsum, lcnt, etab, err_lds, hq, hqv, nq,
                                        epre);
  } else {
    epilogue_generic<BLK>(P, L, cap, nw, log2cap, err_lds, nq);
  }
  if (dbg && threadIdx.x == 0) dbg[blockIdx.x * kDbgPerWg + 3] = __builtin_amdgcn_s_memrealtime();
  if (dbg && (threadIdx.x & 63) == 0) {
    for (int i = 0; i < 6 && DIAG; ++i) dbg[blockIdx.x * kDbgPerWg + 8 + (threadIdx.x >> 6) * 8 + i] = seg[i];
    dbg[blockIdx.x * kDbgPerWg + 8 + (threadIdx.x >> 6) * 8 + 6] = wave_loop_end;
  }
  if constexpr (LEAN) flush_lds_stats(lstat);
  flush_filtered(hq_n);
  flush_wave_stats(n_zero, n_badsvc, n_oor, n_drop);
}

// The small-table kernels by name (sa_path.h SmallKernel): the v2 kernel
// specialised for the default geometry (2,048 slots, 17 buckets, HLL p 14),
// the generic v2 kernel with 512-thread workgroups (two per CU) or 1,024, and
// the linear-threshold kernel for bounds no bin table can hold.
// (the lean window quotient of V2Lean needs window_ns < 2^56, which sa_create
// enforces; SA_OPT_STAMPS engines run the same kernels: the v2 kernels'
// workgroup and wave-end stamps are written whenever P.dbg is set)
constexpr SmallKernel kSmallKernels[] = {SmallKernel::Default, SmallKernel::Generic512, SmallKernel::Generic1024,
                                         SmallKernel::Linear};
static const void *product_small_fn(SmallKernel k) {
  switch (k) {
    case SmallKernel::Default: return (const void *)&ingest_v2_kernel<11, 9, 14, false, 1024, V2Lean>;
    case SmallKernel::Generic512: return (const void *)&ingest_v2_kernel<0, 0, 0, false, 512, V2Lean>;
    case SmallKernel::Generic1024: return (const void *)&ingest_v2_kernel<0, 0, 0, false, 1024, V2Plain>;
    case SmallKernel::Linear: break;
  }
  return (const void *)&ingest_lds_kernel;
}
#ifndef SPANAGG_AB
static const void *small_fn(SmallKernel k, bool) { return product_small_fn(k); }
#else
// + the ablation instance (tools/ablate.py, tools/stamps.py)
#include "lab/small_lab.inc"
#endif

}  // namespace

hipError_t prepare_ingest_small(size_t lds_bytes) {
  for (int diag = 0; diag < 2; ++diag)  // (product build: the same four twice)
    for (SmallKernel k : kSmallKernels)
      if (hipError_t e = hipFuncSetAttribute(small_fn(k, diag), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
          e != hipSuccess)
        return e;
  return hipSuccess;
}

hipError_t launch_ingest_small(const IngestParams &P, uint32_t grid, size_t lds_bytes, hipStream_t s, SmallKernel k,
                               bool diag) {
  void *args[] = {const_cast<IngestParams *>(&P)};
  return hipLaunchKernel(small_fn(k, diag), dim3(grid), dim3(small_block(k)), args, lds_bytes, s);
}

// The same launch as a HIP graph kernel node (sa_ingest_device_many): the
// kernel, its geometry and `args` (args[0] = &P, owned by the caller, read
// when the node is added or its parameters set).
void ingest_small_node(uint32_t grid, size_t lds_bytes, SmallKernel k, void **args, hipKernelNodeParams *np) {
  *np = hipKernelNodeParams{};
  np->func = const_cast<void *>(small_fn(k, false));
  np->gridDim = dim3(grid);
  np->blockDim = dim3(small_block(k));
  np->sharedMemBytes = (unsigned int)lds_bytes;
  np->kernelParams = args;
  np->extra = nullptr;
}

// workgroups of the small-table kernel resident per CU (registers and LDS);
// 0 when the runtime cannot tell.  After prepare_ingest_small.
uint32_t ingest_small_blocks_per_cu(SmallKernel k, bool diag, size_t lds_bytes) {
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, small_fn(k, diag), (int)small_block(k), lds_bytes) != hipSuccess)
    return 0;
  return n > 0 ? (uint32_t)n : 0u;
}

// the EXPO kernel: specialised for the default small table (2,048 slots, HLL
// p = 14: C2's geometry) like SmallKernel::Default, generic otherwise
static const void *expo_small_fn(bool spec) {
  return spec ? (const void *)&ingest_v2_kernel<11, 0, 14, true, 1024, V2Lean>
              : (const void *)&ingest_v2_kernel<0, 0, 0, true, 1024, V2Lean>;
}

hipError_t prepare_ingest_expo_small(size_t lds_bytes) {
  for (bool spec : {false, true})
    if (hipError_t e = hipFuncSetAttribute(expo_small_fn(spec), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        e != hipSuccess)
      return e;
  return hipSuccess;
}
// workgroups of the EXPO kernel resident per CU; 0 when the runtime cannot
// tell.  After prepare_ingest_expo_small.
uint32_t ingest_expo_blocks_per_cu(uint32_t log2cap, uint32_t p, size_t lds_bytes) {
  int n = 0;
  const void *fn = expo_small_fn(expo_kernel(log2cap, p) == ExpoKernel::Specialised);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, (int)kLdsBlock, lds_bytes) != hipSuccess)
    return 0;
  return n > 0 ? (uint32_t)n : 0u;
}

hipError_t launch_ingest_expo_small(const IngestParams &P, uint32_t grid, size_t lds_bytes, hipStream_t s) {
  void *args[] = {const_cast<IngestParams *>(&P)};
  const void *fn = expo_small_fn(expo_kernel(P.log2cap, P.p) == ExpoKernel::Specialised);
  return hipLaunchKernel(fn, dim3(grid), dim3(kLdsBlock), args, lds_bytes, s);
}

}  // namespace sa
