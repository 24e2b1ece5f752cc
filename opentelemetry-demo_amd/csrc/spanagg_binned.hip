// spanagg_binned.hip -- the binned-table high-cardinality path of libspanagg
// (gfx950).  BASELINE config 4: ~1 M series, too many for an LDS-resident key
// table, so every span is first routed to the bin of its series and each bin
// is then aggregated by one workgroup that owns the bin's whole slice of the
// key table and counter rows.  Replaces, for that geometry, the per-span body
// of the connector's aggregateMetrics ([UPSTREAM] spanmetricsconnector
// connector.go: buildKey -> map lookup, Sum.Add(1), explicitHistogram.Observe)
// and adds the sketch updates.
//
// Two kernels per launch:
//   bt_scatter2_kernel<BtHashed> (one 1,024-thread workgroup per CU, ~160 KiB
//   LDS; the template is sa_bt_scatter.h, shared with spanagg_dense.hip, and
//   BtHashed below is this path's part of it)
//     streams the SoA batch once (register tile ring, 16-B nt buffer loads:
//     the C2 kernel's skeleton), does the per-span stats and HLL work, and
//     writes one 16-B record {m's low 53 bits | ERROR flag | window slot,
//     duration} per span into the region of (its bin, this workgroup),
//     through 4-record LDS stages that leave as aligned 64-B chunks.  Hot keys
//     are pre-aggregated in an LDS overflow table; past that, the direct path
//     (key-table CAS + atomics into the spill array).
//   bt_aggregate3_kernel (one 512-thread workgroup per bin; the laboratory
//   build, lab/binned_lab.inc, also keeps bt_aggregate2_kernel, the earlier
//   form, SPANAGG_BT_AGG=2)
//     loads the bin's 2^log2sb key slots into LDS at the same positions,
//     aggregates the bin's records there (u16 bucket-count pairs, u64 ns
//     sums, an ERROR table keyed by (window slot, key slot)), then writes the
//     new keys and read-modify-writes each touched 32-B row of the bin (one
//     owner, no atomics).
// Rows hold u8 bucket counts (sa_internal.h kRowBytes); a count that would
// pass 255 moves the row's counts into the u64 spill array base64.
#include <algorithm>
#include <cstdlib>

#include "sa_bt_scatter.h"

namespace sa {
namespace {

// Find-or-insert m in its bin's sub-table (HBM, CAS); kNotFound when the
// bin is full.  Plain probe reads, as g_find_insert (a stale 0 is corrected
// by the CAS).
__device__ __forceinline__ uint32_t bt_find_insert(unsigned long long *keys, uint64_t m, uint32_t log2sb) {
  const BtSeq q = bt_seq(m, log2sb);
  const uint32_t base = (uint32_t)(m >> kBinShift) << log2sb;
  for (uint32_t i = 0; i < bt_probe_max(log2sb); ++i) {
    const uint32_t s = base | bt_pos(q, i);
    unsigned long long k = keys[s];
    if (k == m) return s;
    if (k == 0) {
      const unsigned long long prev = atomicCAS(&keys[s], 0ULL, (unsigned long long)m);
      if (prev == 0 || prev == m) return s;
    }
  }
  return kNotFound;
}

// Adds cnt spans of bucket bk and an ns sum to key slot s in the u64 spill
// array with atomics (the direct path and the overflow table's rows).
__device__ __forceinline__ void spill_add(unsigned long long *base64, uint32_t nbk, uint32_t s, uint32_t bk,
                                          uint32_t cnt, unsigned long long dsum) {
  unsigned long long *row = base64 + (uint64_t)s * (nbk + 1);
  if (cnt) atomicAdd(row + bk, (unsigned long long)cnt);
  if (dsum) atomicAdd(row + nbk, dsum);
}

// Count-min cells of one ERROR span without a key-table slot (d atomics).
template <typename QP>
__device__ __forceinline__ void bt_cms_add(QP Q, uint32_t ws, uint64_t key) {
  SA_GLOBAL unsigned long long *row0 = gbl(Q->cms) + (uint64_t)ws * Q->cms_d * Q->cms_w;
  for (uint32_t r = 0; r < Q->cms_d; ++r) {
    const uint64_t col = splitmix64(key ^ Q->seeds[r]) >> Q->cms_shift;
    __hip_atomic_fetch_add(row0 + (uint64_t)r * Q->cms_w + col, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Cold paths of the scatter.
__device__ __noinline__ void bt_cold_err(KParams Q, uint64_t m, uint32_t ws) {
  const uint32_t s = bt_find_insert(Q->gkeys, m, Q->log2sb);
  if (s != kNotFound) atomicAdd(Q->errcnt + ((uint64_t)ws << Q->log2cap) + s, 1ULL);
  else bt_cms_add(Q, ws, m * Q->kinv);
}

// returns 1 when the span was dropped (its bin is full)
__device__ __noinline__ uint32_t bt_cold_direct(KParams Q, uint64_t m, uint64_t d, uint32_t bk, bool err,
                                                uint32_t ws) {
  const uint32_t s = bt_find_insert(Q->gkeys, m, Q->log2sb);
  if (s == kNotFound) {
    if (err) bt_cms_add(Q, ws, m * Q->kinv);
    return 1u;
  }
  spill_add(Q->base64, Q->nbk, s, bk, 1u, d);
  if (err) atomicAdd(Q->errcnt + ((uint64_t)ws << Q->log2cap) + s, 1ULL);
  return 0u;
}

// The scatter's Path (sa_bt_scatter.h) for series given by hash.  The id is
// m = key * kmul (its top bits pick the bin; key 0 has no record); a record
// is 16 B {m's low 53 bits | ERROR flag | window slot, duration | bucket}, in
// 4-record stages.  A span past the overflow table takes the key-table path
// (find-or-insert, atomics into the spill array; count-min when the bin is
// full, the span then counted as dropped), and the epilogue looks every
// overflow-table entry up the same way.
struct BtHashed {
  typedef uint64_t Id;
  typedef ulonglong2 Rec;
  static constexpr uint32_t kStage = kBtStage;
  static constexpr uint64_t kDurMask = kRecDurMask;
  static constexpr uint32_t kBinLsb = kBinShift;
  static constexpr bool kStamps = true, kLookup = true, kClampDrain = false;
  static __device__ __forceinline__ Id id(const IngestParams &P, uint64_t key, uint32_t &, uint64_t) {
    return key * P.kmul;
  }
  static __device__ __forceinline__ uint32_t home_hash(Id m) { return (uint32_t)(m >> 21); }
  static __device__ __forceinline__ Rec rec(Id m, uint64_t d, uint32_t bk, bool err, uint32_t ws) {
    return make_ulonglong2((m & kBinRest) | (err ? (1ULL << 63) | ((uint64_t)ws << kBinShift) : 0ULL),
                           d | ((uint64_t)bk << kRecDurBits));
  }
  static __device__ __forceinline__ Id rec_id(uint32_t b, const Rec &r) {
    return ((uint64_t)b << kBinShift) | (r.x & kBinRest);
  }
  static __device__ __forceinline__ uint64_t rec_d(const Rec &r) { return r.y & kRecDurMask; }
  static __device__ __forceinline__ bool rec_err(const Rec &r) { return (r.x >> 63) != 0; }
  static __device__ __forceinline__ uint32_t rec_ws(const Rec &r) { return (uint32_t)(r.x >> kBinShift) & 1023u; }
  static __device__ __forceinline__ bool same_id(const Rec &a, const Rec &b) { return ((a.x ^ b.x) & kBinRest) == 0; }
  // the cold paths take the id; cold_direct returns 1 when the span was dropped
  static __device__ __forceinline__ Id cold_key(const IngestParams &, Id m) { return m; }
  static __device__ __forceinline__ uint32_t cold_direct(KParams kp, Id m, uint64_t d, uint32_t bk, bool err,
                                                         uint32_t ws) {
    return bt_cold_direct(kp, m, d, bk, err, ws);
  }
  static __device__ __forceinline__ void cold_err(KParams kp, Id m, uint32_t ws) { bt_cold_err(kp, m, ws); }
  static __device__ __forceinline__ uint32_t lookup(const IngestParams &P, Id m) {
    return bt_find_insert(P.gkeys, m, P.log2sb);
  }
  // one ERROR span of an overflow-table entry whose bin is full
  static __device__ __forceinline__ void err_no_row(KParams kp, const IngestParams &P, Id m, uint32_t ws) {
    bt_cms_add(kp, ws, m * P.kinv);
  }
};

// Aggregate geometry (bt_aggregate3_kernel; the laboratory build's earlier
// form bt_aggregate2_kernel shares it).  One 512-thread workgroup per bin;
// its LDS holds the bin's key slots (mirror), u64 ns sums and u16 bucket
// counts (17 per slot, packed), an ERROR table and the region fills: 53 KiB
// at 1,024 slots, so three workgroups share a CU.  No prefix scan: each
// wave-instruction reads two regions (lanes 0-31 and 32-63, one record per
// lane), a wave takes every eighth region pair and issues its loads in
// batches of eight before it aggregates them.  Then each touched slot's u32
// row is read, added to and written back (all reads first).
constexpr uint32_t kBtAgg2Block = 512;
constexpr uint32_t kBtAgg2Err = 128;
__host__ __device__ inline uint32_t bt_agg2_cnt_words(uint32_t sb) { return (sb * kPartMaxBk + 1) / 2; }
__host__ __device__ inline uint32_t bt_agg2_off_err(uint32_t sb) { return (sb * 16 + bt_agg2_cnt_words(sb) * 4 + 7) & ~7u; }
__host__ __device__ inline uint32_t bt_agg2_off_reg(uint32_t sb) { return bt_agg2_off_err(sb) + kBtAgg2Err * 8; }



// Aggregate, third form (the default).  The layout, phases and row
// write-back of bt_aggregate2_kernel; the records go through the LDS two per
// lane at a time with every LDS access of the pair issued before the first
// one is waited for -- both records' two key buckets (4 x ds_read_b128 each),
// then the compares, then both records' counter atomics -- instead of one
// record's dependent chain after another (a record costs ~6 LDS round trips
// in sequence there).  Records carry their bucket (the scatter's bin table),
// so there is no per-record bucketing.  A key missing from its two buckets
// (new in the bin, or placed past them) takes the probe loop, rare after the
// first launches.  ERROR records append (window slot, key slot) to an LDS
// list, added to errcnt after the records (global atomics past the list's
// 255).  The record loop keeps its VALU lean -- 32-bit key arithmetic
// (records carry m's low 53 bits, so m's high word is (x.hi & 0x1FFFFF) |
// bin << 21), load offsets stepped per batch, the in-bucket slot picked as an
// index 0-7 by inline-constant selects -- and its batches of two region pairs
// are double-buffered: the next batch's loads are issued before this one goes
// through the LDS.
// MODE (ablation): 1 = no records aggregated, 2 = no key / row write-back,
// 16 = no lookup reads, 32 = no counter atomics.
template <int MODE = 0, int MAXPER = 2, int BLOCK = 512>
__global__ __launch_bounds__(BLOCK, BLOCK == 1024 ? 8 : 6) void bt_aggregate3_kernel(IngestParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t log2sb = P.log2sb, sb = 1u << log2sb;
  // record sets: one, or two (P.bt_rec2: two launches' scatters aggregated
  // together, so the bin's setup and row write-back serve both)
  const uint32_t nrs = cold_params().bt_rec2 ? 2u : 1u;
  const uint32_t Gmax = nrs == 2 && cold_params().bt_grid2 > P.bt_grid ? cold_params().bt_grid2 : P.bt_grid;
  const uint32_t bin = blockIdx.x;
  unsigned long long *lkeys = reinterpret_cast<unsigned long long *>(smem);
  unsigned long long *lsum = lkeys + sb;
  uint32_t *lcnt = reinterpret_cast<uint32_t *>(lsum + sb);  // u16 [sb][17], packed
  constexpr uint32_t kErrL = kBtAgg2Err * 2;                  // u32 words in the etab space
  uint32_t *errl = reinterpret_cast<uint32_t *>(smem + bt_agg2_off_err(sb));  // [0] count, [1..] ek + 1
  uint32_t *rcnt = reinterpret_cast<uint32_t *>(smem + bt_agg2_off_reg(sb));  // [G] region fills (the set's)
  uint32_t *misc = rcnt + Gmax;  // [0] dropped
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  unsigned long long *gk = P.gkeys + ((uint64_t)bin << log2sb);
  bt_stamp(P, (uint64_t)bin * 8, 0);

  // 1. the bin's key slots (kept in registers to find the new ones later),
  //    region fills, zeroed counters
  constexpr int kMaxPer = MAXPER;
  unsigned long long orig[kMaxPer];
#pragma unroll
  for (int u = 0; u < kMaxPer; ++u) {
    const uint32_t s = tid + u * BLOCK;
    orig[u] = s < sb ? gk[s] : 0ULL;
  }
  for (uint32_t g = tid; g < P.bt_grid; g += BLOCK) rcnt[g] = P.bt_cnt[(uint64_t)bin * P.bt_grid + g];
#pragma unroll
  for (int u = 0; u < kMaxPer; ++u) {
    const uint32_t s = tid + u * BLOCK;
    if (s < sb) {
      lkeys[s] = orig[u];
      lsum[s] = 0;
    }
  }
  const uint32_t cw = bt_agg2_cnt_words(sb);
  for (uint32_t i = tid; i < cw; i += BLOCK) lcnt[i] = 0;
  if (tid == 0) errl[0] = misc[0] = 0;
  __syncthreads();
  bt_stamp(P, (uint64_t)bin * 8, 1);

  // 2. the records, set by set
  const uint32_t half = lane >> 5, r0 = lane & 31u;
  const uint32_t pmax = bt_probe_max(log2sb);
  uint32_t n_drop = 0;
  const ulonglong2 *lk2 = reinterpret_cast<const ulonglong2 *>(lkeys);
  const uint32_t binhi = bin << (kBinShift - 32);
  const uint32_t sh = 34 - log2sb;  // bt_seq: the top (log2sb - 2) bits
  // two records (ok: valid) through the LDS together
  auto agg_pair = [&](const ulonglong2 (&v)[2], const bool (&ok)[2]) {
    uint32_t mlo[2], mhi[2], b1[2], b2[2];
    ulonglong2 q[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      mlo[k] = (uint32_t)v[k].x;
      mhi[k] = (((uint32_t)(v[k].x >> 32)) & ((1u << (kBinShift - 32)) - 1)) | binhi;
      // bt_seq on the 32-bit halves
      const uint32_t h1 = (mlo[k] ^ __builtin_amdgcn_alignbit(mhi[k], mlo[k], 29)) * 0x9E3779B1u;
      const uint32_t h2 = (h1 ^ (h1 >> 16)) * 0x85EBCA6Bu;
      b1[k] = h1 >> sh;
      b2[k] = h2 >> sh;
      if (MODE & 16) {  // ablation: no lookup reads (every key taken as slot 0 of its first bucket)
        q[k][0] = make_ulonglong2(((uint64_t)mhi[k] << 32) | mlo[k], 0);
        q[k][1] = q[k][2] = q[k][3] = make_ulonglong2(0, 0);
        continue;
      }
      q[k][0] = lk2[b1[k] * 2];
      q[k][1] = lk2[b1[k] * 2 + 1];
      q[k][2] = lk2[b2[k] * 2];
      q[k][3] = lk2[b2[k] * 2 + 1];
    }
    // position in the two buckets (8: not there)
    uint32_t s[2], j[2] = {8u, 8u};
    uint64_t mm[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) mm[k] = ((uint64_t)mhi[k] << 32) | mlo[k];
#pragma unroll
    for (int i = 7; i >= 0; --i) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const unsigned long long w = (i & 1) ? q[k][i >> 1].y : q[k][i >> 1].x;
        j[k] = w == mm[k] ? (uint32_t)i : j[k];
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const uint32_t sl = ((j[k] < 4 ? b1[k] : b2[k]) << 2) | (j[k] & 3u);
      s[k] = j[k] < 8 ? sl : kNotFound;
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (__builtin_expect(ok[k] && s[k] == kNotFound, 0)) {  // probe / insert in the mirror
        const BtSeq bq = bt_seq(mm[k], log2sb);
        uint32_t i = 0, sl = kNotFound;
        for (; i < pmax; ++i) {
          sl = bt_pos(bq, i);
          unsigned long long kk = lkeys[sl];
          if (kk == 0) kk = atomicCAS(&lkeys[sl], 0ULL, (unsigned long long)mm[k]);
          if (kk == 0 || kk == mm[k]) break;
        }
        s[k] = i == pmax ? kNotFound - 1 : sl;  // kNotFound - 1: the bin's sub-table is full
      }
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (!ok[k]) continue;
      const uint32_t xhi = (uint32_t)(v[k].x >> 32);
      const bool err = (int32_t)xhi < 0;
      const uint32_t ws = (xhi >> (kBinShift - 32)) & 1023u;
      if (__builtin_expect(s[k] == kNotFound - 1, 0)) {  // dropped
        ++n_drop;
        if (err) bt_cms_add(kernel_params(), ws, mm[k] * P.kinv);
        continue;
      }
      const uint32_t yhi = (uint32_t)(v[k].y >> 32);
      uint32_t h;  // the (slot, bucket) u16 counter: s * 17 + bucket
      asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(h) : "v"(s[k]), "i"(kPartMaxBk), "v"(yhi >> (kRecDurBits - 32)));
      if (MODE & 32) {  // ablation: no counter atomics
        n_drop += (h == 0xFFFFFFFu) ? 1u : 0u;
      } else {
        atomicAdd(&lcnt[h >> 1], 1u << ((h & 1u) << 4));
        atomicAdd(&lsum[s[k]], ((unsigned long long)(yhi & ((1u << (kRecDurBits - 32)) - 1)) << 32) | (uint32_t)v[k].y);
      }
      if (err) {
        const uint32_t ek = (ws << log2sb) | s[k];
        const uint32_t at = atomicAdd(&errl[0], 1u);
        if (at + 1 < kErrL) errl[at + 1] = ek;
        // past the LDS list: the key's canonical HBM slot (find-or-insert), so
        // the count stays right if the write-back relocates the key
        else bt_cold_err(kernel_params(), mm[k], ws);
      }
    }
  };
  constexpr uint32_t kWaves = BLOCK / 64;
#pragma unroll 1
  for (uint32_t rs = 0; rs < nrs; ++rs) {
    // (the second set's parameters through the kernarg pointer: read where
    // they are used, so they hold no scalar registers across the first set)
    SA_CONST const IngestParams &Q = cold_params();
    const uint32_t G = rs ? Q.bt_grid2 : P.bt_grid, region = rs ? Q.bt_region2 : P.bt_region;
    if (rs) {  // the second set's region fills (every wave is past the first set's records)
      __syncthreads();
      for (uint32_t g = tid; g < G; g += BLOCK) rcnt[g] = Q.bt_cnt2[(uint64_t)bin * G + g];
      __syncthreads();
    }
    const ulonglong2 *bin_rec = (rs ? Q.bt_rec2 : P.bt_rec) + (uint64_t)bin * G * region;
    const __amdgpu_buffer_rsrc_t rrec = rsrc(bin_rec, G * region * 16);
    const uint32_t pairs = (G + 1) / 2;
    if (!(MODE & 1)) {
      // the wave's region pairs p = wave + 8 j; this lane's region g = 2 p +
      // half, its byte offset stepped by 16 regions per pair.  Batches of two
      // pairs, double-buffered (a batch past the bin's regions loads nothing
      // and adds nothing).
      const uint32_t g0 = 2 * wave + half;
      const uint32_t rstep = 2 * kWaves * region * 16;
      uint32_t roff = (g0 * region + r0) * 16;
      uint32_t goff = g0;
      auto issue = [&](ulonglong2 (&v)[2], bool (&ok)[2]) {
#pragma unroll
        for (uint32_t b = 0; b < 2; ++b) {
          const uint32_t g = goff + b * 2 * kWaves;
          const uint32_t c = rcnt[g < G ? g : 0u];
          ok[b] = g < G && r0 < c;
          const auto x = __builtin_amdgcn_raw_buffer_load_b128(rrec, (int)(ok[b] ? roff + b * rstep : 0xFFFFFFF0u), 0, 2);
          v[b] = make_ulonglong2((uint64_t)x[0] | ((uint64_t)x[1] << 32), (uint64_t)x[2] | ((uint64_t)x[3] << 32));
        }
        roff += 2 * rstep;
        goff += 4 * kWaves;
      };
      ulonglong2 va[2], vb[2];
      bool oka[2], okb[2];
      issue(va, oka);
      for (uint32_t p0 = wave; p0 < pairs; p0 += kWaves * 4) {
        issue(vb, okb);
        agg_pair(va, oka);
        issue(va, oka);
        agg_pair(vb, okb);
      }
      // regions longer than 32 records: the rest, one record per lane
#pragma unroll 1
      for (uint32_t p = wave; p < pairs; p += kWaves) {
        const uint32_t g = 2 * p + half;
        const uint32_t c = g < G ? rcnt[g] : 0u;
        for (uint32_t r = 32 + r0; r < c; r += 32) {
          const ulonglong2 vv[2] = {bin_rec[(uint64_t)g * region + r], make_ulonglong2(0, 0)};
          const bool ok[2] = {true, false};
          agg_pair(vv, ok);
        }
      }
    }
  }
  // the rows of the slots the bin held at setup, loaded by each wave right
  // after its records, before the barrier: waves end their records at
  // different times, so these loads land while the last ones work, and the
  // write-back below reads HBM only for keys new to the bin (a slot that held
  // a key keeps it; the rows are this aggregate's alone)
  uint4 *rows = reinterpret_cast<uint4 *>(P.gcounts) + ((uint64_t)bin << log2sb) * (kRowBytes / 16);
  uint4 rpre[kMaxPer][2];
#pragma unroll
  for (int u = 0; u < kMaxPer; ++u) {
    const uint32_t s = tid + u * BLOCK;
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q)
      rpre[u][q] = s < sb && orig[u] != 0 && !(MODE & 2) ? rows[(uint64_t)s * 2 + q] : make_uint4(0, 0, 0, 0);
  }
  n_drop = wave_sum(n_drop);
  if (lane == 0 && n_drop) atomicAdd(&misc[0], n_drop);
  __syncthreads();
  bt_stamp(P, (uint64_t)bin * 8, 2);

  // 3. new keys and touched rows of the bin (one owner: plain stores; every
  //    row read is issued before the first row is written); the ERROR list.
  //    The next launch's scatter may run beside this aggregate (the engine
  //    overlaps them, section "launch pipeline" of spanagg_engine.cpp) and
  //    CAS-insert keys into this bin's HBM sub-table meanwhile, so a key this
  //    aggregate added to its LDS mirror is inserted into HBM by the same
  //    find-or-insert the scatter uses: slots never empty and every inserter
  //    probes one sequence, so the HBM table stays free of duplicates.  When
  //    the key lands in another slot than its LDS one (a concurrent insert
  //    took that slot or an earlier one of the key's sequence), its counts go
  //    to that slot's spill-array cells by atomics and the LDS slot's row is
  //    left alone; lsum[s] then carries the relocated slot for the ERROR list.
  if (MODE & 2) return;
  const uint32_t nbk = P.nbk;
  constexpr unsigned long long kMoved = 1ULL << 63;  // lsum[s] after the write-back: kMoved | new slot (or kNotFound)
  uint4 rv[kMaxPer][2];
  bool touched[kMaxPer];
  uint32_t hs[kMaxPer];  // the HBM slot (in the whole table) holding lkeys[s]
#pragma unroll
  for (int u = 0; u < kMaxPer; ++u) {
    const uint32_t s = tid + u * BLOCK;
    hs[u] = (bin << log2sb) | s;
    if (s < sb && lkeys[s] != orig[u]) {
      const uint32_t f = bt_find_insert(P.gkeys, lkeys[s], log2sb);
      hs[u] = f;  // kNotFound: the bin's HBM sub-table filled meanwhile
    }
    touched[u] = s < sb && lsum[s] != 0;
    if (s < sb && !touched[u]) {  // a zero ns sum: look at the counts
      uint32_t any = 0;
      for (uint32_t b = 0; b < nbk; ++b) {
        const uint32_t h = s * kPartMaxBk + b;
        any |= (lcnt[h >> 1] >> ((h & 1u) * 16)) & 0xFFFFu;
      }
      touched[u] = any != 0;
    }
    const bool own = hs[u] == ((bin << log2sb) | s);
#pragma unroll
    for (uint32_t q = 0; q < 2; ++q)
      rv[u][q] = !(touched[u] && own) ? make_uint4(0, 0, 0, 0)
                 : orig[u] != 0  ? rpre[u][q]
                                 : rows[(uint64_t)s * 2 + q];
  }
  uint32_t n_lost = 0;
#pragma unroll
  for (int u = 0; u < kMaxPer; ++u) {
    const uint32_t s = tid + u * BLOCK;
    if (s >= sb) continue;
    const bool own = hs[u] == ((bin << log2sb) | s);
    const unsigned long long ls = lsum[s];
    lsum[s] = own ? 0ULL : kMoved | hs[u];
    if (!touched[u]) continue;
    if (!own) {  // relocated (or lost): the counts by atomics into the spill array
      for (uint32_t b = 0; b < nbk; ++b) {
        const uint32_t h = s * kPartMaxBk + b;
        const uint32_t c = (lcnt[h >> 1] >> ((h & 1u) * 16)) & 0xFFFFu;
        if (hs[u] == kNotFound) n_lost += c;
        else if (c) atomicAdd(P.base64 + (uint64_t)hs[u] * (nbk + 1) + b, (unsigned long long)c);
      }
      if (hs[u] != kNotFound && ls) atomicAdd(P.base64 + (uint64_t)hs[u] * (nbk + 1) + nbk, ls);
      continue;
    }
    const uint32_t w[8] = {rv[u][0].x, rv[u][0].y, rv[u][0].z, rv[u][0].w,
                           rv[u][1].x, rv[u][1].y, rv[u][1].z, rv[u][1].w};
    const unsigned long long sum = ((unsigned long long)w[1] << 32 | w[0]) + ls;  // (lsum[s] now holds the relocation mark)
    uint32_t c[kPartMaxBk];
    bool spill = false;
#pragma unroll
    for (uint32_t b = 0; b < kPartMaxBk; ++b) {
      const uint32_t h = s * kPartMaxBk + b;
      c[b] = b < nbk ? ((w[2 + b / 4] >> ((b & 3u) * 8)) & 0xFFu) + ((lcnt[h >> 1] >> ((h & 1u) * 16)) & 0xFFFFu)
                     : 0u;
      spill |= c[b] > 0xFFu;
    }
    uint32_t o[6] = {0, 0, 0, 0, 0, 0};
    if (spill) {  // the row's counts move to the spill array (atomics: the scatter adds there too)
      unsigned long long *sp = P.base64 + ((uint64_t)bin << log2sb | s) * (nbk + 1);
#pragma unroll
      for (uint32_t b = 0; b < kPartMaxBk; ++b)
        if (c[b]) atomicAdd(sp + b, (unsigned long long)c[b]);
    } else {
#pragma unroll
      for (uint32_t b = 0; b < kPartMaxBk; ++b) o[b / 4] |= c[b] << ((b & 3u) * 8);
    }
    rows[(uint64_t)s * 2] = make_uint4((uint32_t)sum, (uint32_t)(sum >> 32), o[0], o[1]);
    rows[(uint64_t)s * 2 + 1] = make_uint4(o[2], o[3], o[4], o[5]);
  }
  n_lost = wave_sum(n_lost);
  if (lane == 0 && n_lost) atomicAdd(&misc[0], n_lost);
  __syncthreads();  // lsum carries the relocations for the ERROR list
  const uint32_t ne = min(errl[0], kErrL - 1);
  for (uint32_t i = tid; i < ne; i += BLOCK) {
    const uint32_t ek = errl[i + 1], ws = ek >> log2sb, s = ek & (sb - 1);
    const unsigned long long mv = lsum[s];
    const uint32_t slot = (mv & kMoved) ? (uint32_t)mv : ((bin << log2sb) | s);
    if (slot != kNotFound) atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + slot, 1ULL);
    else bt_cms_add(kernel_params(), ws, lkeys[s] * P.kinv);
  }
  if (tid == 0 && misc[0]) atomicAdd(&P.stats[kStatDropped], (unsigned long long)misc[0]);
  bt_stamp(P, (uint64_t)bin * 8, 3);
}

}  // namespace

#ifdef SPANAGG_AB
// the laboratory build's earlier aggregate form, ablation instances and
// kernel selection (tools/ A/B runs; never in libspanagg.so)
#include "lab/binned_lab.inc"
#else
// Product build: one scatter and one aggregate (bins of up to 1,024 slots, or
// the wide form for 2,048).
static const void *bt_scatter2_fn(uint32_t) { return (const void *)&bt_scatter2_kernel<BtHashed, 0>; }
constexpr uint32_t kDiagBtAggWide = 1u << 30;
static const void *bt_agg_fn(uint32_t diag) {
  return (diag & kDiagBtAggWide) ? (const void *)&bt_aggregate3_kernel<0, 4> : (const void *)&bt_aggregate3_kernel<0, 2>;
}
hipError_t prepare_ingest_bt(size_t agg_lds) {
  if (hipError_t e = hipFuncSetAttribute(bt_scatter2_fn(0), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kBt2ScatterLds);
      e != hipSuccess)
    return e;
  for (uint32_t v : {0u, kDiagBtAggWide})
    if (hipError_t e = hipFuncSetAttribute(bt_agg_fn(v), hipFuncAttributeMaxDynamicSharedMemorySize, (int)agg_lds);
        e != hipSuccess)
      return e;
  return hipSuccess;
}
constexpr uint32_t kDiagBtNoScatter = 0, kDiagBtNoAgg = 0;
static uint32_t bt_agg_block() { return kBtAgg2Block; }
#endif

hipError_t launch_bt_scatter(const IngestParams &P, hipStream_t s) {
  if (P.diag & kDiagBtNoScatter) return hipSuccess;
  void *args[] = {const_cast<IngestParams *>(&P)};
  return hipLaunchKernel(bt_scatter2_fn(P.diag), dim3(P.bt_grid), dim3(kBtBlock), args, kBt2ScatterLds, s);
}

hipError_t launch_bt_aggregate(const IngestParams &P, hipStream_t s) {
  if (P.diag & kDiagBtNoAgg) return hipSuccess;
  void *args[] = {const_cast<IngestParams *>(&P)};
  const uint32_t diag = P.diag | (P.log2sb > 10 ? kDiagBtAggWide : 0u);
  // (two record sets: the region-fill array holds the larger set's)
  const uint32_t g = P.bt_rec2 && P.bt_grid2 > P.bt_grid ? P.bt_grid2 : P.bt_grid;
  return hipLaunchKernel(bt_agg_fn(diag), dim3(kPartBins), dim3(bt_agg_block()), args, bt_agg2_lds_bytes(P.log2sb, g),
                         s);
}

size_t bt_agg2_lds_bytes(uint32_t log2sb, uint32_t grid) {
  return bt_agg2_off_reg(1u << log2sb) + (size_t)grid * 4 + 16;
}

}  // namespace sa
