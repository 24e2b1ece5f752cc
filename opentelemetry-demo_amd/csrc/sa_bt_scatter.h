// sa_bt_scatter.h -- the scatter kernel of the binned high-cardinality path of
// libspanagg (gfx950), one template for its two forms: spanagg_binned.hip
// instantiates it with BtHashed (series given by their 64-bit hash, rows found
// by find-or-insert), spanagg_dense.hip with BtDense (series given by a dense
// index, rows by arithmetic).  Everything the two share -- LDS layout,
// register tile ring, per-span stats and HLL, stages and their flush, the
// overflow table, region fills, the epilogue -- is written here once; a Path
// carries only what differs:
//   Rec, kStage       the record type and the records per bin stage (a stage
//                     is one aligned 64-B chunk: 64 / kStage lanes flush one)
//   Id, id()          a span's series id from its key column (0: no record;
//                     id() may count a key it refuses in n_drop)
//   kBinLsb           the bin of an id: its kPartBinBits bits from this one up
//                     (a constant, not an accessor: bin(id) as a function
//                     costs the dense instance 12 more spilled VGPRs)
//   home_hash(), rec(), rec_id/d/err/ws(), same_id(), kDurMask
//                     the overflow-table home, the record's encoding, its
//                     same-series test and duration limit
//   cold_key(), cold_direct(), cold_err()
//                     the per-span paths past the overflow table, and what
//                     they take (the id or its row)
//   kLookup, lookup() / row()
//                     how an overflow-table entry finds its row in the
//                     epilogue: a find-or-insert pass, or arithmetic
//   kStamps, kClampDrain
//                     diagnostic timestamps; the partial-stage drain's clamp
#pragma once
#include "sa_device.h"

namespace sa {
namespace {

// Diagnostic per-workgroup timestamps (SPANAGG_STAMPS builds of the engine):
// s_memrealtime (100 MHz, comparable across CUs) into dbg[base + k].
__device__ __forceinline__ void bt_stamp(const IngestParams &P, uint64_t base, uint32_t k) {
  if (P.dbg && threadIdx.x == 0) P.dbg[base + k] = __builtin_amdgcn_s_memrealtime();
}

// Count-min cells of one ERROR span whose key column is 0 (d atomics; cold).
__device__ __noinline__ void bt_err_no_series(KParams Q, uint32_t ws) {
  SA_GLOBAL unsigned long long *row0 = gbl(Q->cms) + (uint64_t)ws * Q->cms_d * Q->cms_w;
  for (uint32_t r = 0; r < Q->cms_d; ++r) {
    const uint64_t col = splitmix64(Q->seeds[r]) >> Q->cms_shift;  // (key 0 ^ seed)
    __hip_atomic_fetch_add(row0 + (uint64_t)r * Q->cms_w + col, 1ULL, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Round-synchronous scatter.  The workgroup takes its span range in rounds of
// 2,048 spans (one 128-span tile per wave, two rounds of tiles in flight);
// every span claims a slot of its bin's kStage-record LDS stage with one LDS
// atomic.  After a barrier each wave collects the full stages of the 128 bins
// it owns into a list and writes them out 64 / kStage lanes per stage, so every
// stage leaves as one aligned 64-B piece of a single store instruction; a
// second barrier frees the stages for the next round.  Ids already in the
// overflow table (the hot series of a skewed mix) are added there directly;
// a span whose stage is full in its round, or whose region is used up, goes
// to the overflow table, past that the Path's direct path.  The records of a
// (bin, workgroup) region are the ones the Path's aggregate kernel reads.
// u16 counters: a workgroup takes at most kBtMaxWgSpans (65,520) spans per
// launch, which bounds its region claims per bin and every overflow-table
// count.
// MODE (ablation, laboratory build): 1 = no records, 2 = no HLL, 4 =
// overflow-table adds skipped, 8 = overflow-table ERROR counts skipped, 16 =
// no scatter, 32 = no store, 64 = a flush every second round from the start.
template <class Path, int MODE = 0>
__global__ __launch_bounds__(kBtBlock) void bt_scatter2_kernel(IngestParams P) {
  using Id = typename Path::Id;
  using Rec = typename Path::Rec;
  constexpr uint32_t kStage = Path::kStage;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t kWaves = kBtBlock / 64;
  Rec *stage = reinterpret_cast<Rec *>(smem);                                        // [bins][kStage]
  uint32_t *fillw = reinterpret_cast<uint32_t *>(stage + kPartBins * kStage);        // [bins / 2] u16 pairs
  uint32_t *rcnw = fillw + kPartBins / 2;                                            // [bins / 2] region fills
  uint16_t *flist = reinterpret_cast<uint16_t *>(rcnw + kPartBins / 2);              // [waves][128]
  unsigned long long *hkey = reinterpret_cast<unsigned long long *>(flist + kWaves * 128);  // the entry's id
  unsigned long long *hsum = hkey + kBt2Hot;
  uint32_t *hcnt = reinterpret_cast<uint32_t *>(hsum + kBt2Hot);  // [kBt2Hot][kPartWords] u16 pairs
  uint2 *hq = reinterpret_cast<uint2 *>(hcnt + kBt2Hot * kPartWords);
  uint32_t *hq_n = reinterpret_cast<uint32_t *>(hq + kBtHq);
  BinEntry *lbins = reinterpret_cast<BinEntry *>(hq_n + 4);
  uint2 *herr = reinterpret_cast<uint2 *>(lbins + kBins);  // [kBt2HotErr] {(ws << 8 | entry) + 1, count}
  uint8_t *llb = reinterpret_cast<uint8_t *>(herr + kBt2HotErr);
  const KParams kp = kernel_params();
  const uint64_t sbase = (uint64_t)kPartBins * 8 + blockIdx.x * 8;
  auto stamp = [&](uint32_t k) {
    if constexpr (Path::kStamps) bt_stamp(P, sbase, k);
  };
  stamp(0);

  uint64_t lo, hi;
  wg_range_p(P, lo, hi);
  const uint32_t len = (uint32_t)(hi - lo);
  constexpr uint32_t kRound = kBtBlock * 2;
  const uint32_t lane = threadIdx.x & 63u, lane_off = lane * 2;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t rounds = (len + kRound - 1) / kRound;
  auto tstart = [&](uint32_t r) -> uint32_t { return r * kRound + wave * 128; };
  auto tremain = [&](uint32_t t) -> uint32_t { return len > t ? len - t : 0u; };

  // prologue: bin table and bounds, the first two rounds' tiles, LDS setup
  uint4 bv = make_uint4(0, 0, 0, 0);
  if (threadIdx.x < kBins * 2) bv = reinterpret_cast<const uint4 *>(P.bintab)[threadIdx.x];
  const uint32_t lb_on = P.lb_n != 0 && !(MODE & 2);
  uint32_t lbw = 0;
  if (lb_on && threadIdx.x * 4 < P.lb_n) lbw = *reinterpret_cast<const uint32_t *>(P.hll_lb + threadIdx.x * 4);
  SpanTile<2> buf[2];
  Pending<2> pend, pend2;  // HLL reads of the last two rounds (compared two rounds later:
                           // the flush stores between a read and its compare would
                           // otherwise make that wait drain the prefetched tiles too)
  load_tile_at<2, 2>(P, lo + tstart(0), tremain(tstart(0)), lane_off, buf[0]);
  load_tile_at<2, 2>(P, lo + tstart(1), tremain(tstart(1)), lane_off, buf[1]);
  {
    uint32_t z;  // a VGPR zero keeps these vector loads
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
#pragma unroll
    for (int j = 0; j < 2; ++j) pend.hv[j] = pend2.hv[j] = *reinterpret_cast<const uint32_t *>(P.hll + z);
  }
  for (uint32_t b = threadIdx.x; b < kPartBins / 2; b += kBtBlock) fillw[b] = rcnw[b] = 0;
  for (uint32_t h = threadIdx.x; h < kBt2Hot; h += kBtBlock) hkey[h] = hsum[h] = 0;
  for (uint32_t h = threadIdx.x; h < kBt2Hot * kPartWords; h += kBtBlock) hcnt[h] = 0;
  if (threadIdx.x < kBt2HotErr) herr[threadIdx.x] = make_uint2(0, 0);
  if (threadIdx.x < kBins * 2) reinterpret_cast<uint4 *>(lbins)[threadIdx.x] = bv;
  if (lb_on && threadIdx.x * 4 < P.lb_n) reinterpret_cast<uint32_t *>(llb)[threadIdx.x] = lbw;
  if (threadIdx.x == 0) hq_n[0] = 0;
  __syncthreads();
  stamp(1);

  uint32_t n_zero = 0, n_badsvc = 0, n_oor = 0;  // wave-uniform (SGPR)
  uint32_t n_drop = 0;                           // per lane
  uint32_t n_filt = 0;                           // per lane: HLL updates the lower-bound filter skipped
#pragma unroll
  for (int j = 0; j < 2; ++j) pend.hoff[j] = pend.rho[j] = pend2.hoff[j] = pend2.rho[j] = 0;
  const uint32_t region = P.bt_region;
  Rec *my_rec = reinterpret_cast<Rec *>(P.bt_rec) + (uint64_t)blockIdx.x * region;  // + bin * grid * region
  const uint64_t bin_stride = (uint64_t)P.bt_grid * region;
  const uint64_t cap = 1ULL << P.log2cap;  // the table's slots (for Path::id)

  // overflow-table home: an even entry, probed as a pair first
  auto hot_home = [&](Id id) -> uint32_t {
    return (uint32_t)(((uint64_t)Path::home_hash(id) * (kBt2Hot / 2)) >> 32) * 2;
  };
  auto hot_acc = [&](uint32_t h, Id id, uint64_t d, bool err, uint32_t ws) {
    if (MODE & 4) return;
    const uint32_t bk = bucket_lds<1>(d, lbins, P);
    atomicAdd(&hcnt[h * kPartWords + (bk >> 1)], 1u << ((bk & 1u) * 16));
    atomicAdd(&hsum[h], (unsigned long long)d);
    if (err && !(MODE & 8)) {  // ERROR count per (window slot, entry); a full table takes the Path's cold path
      const uint32_t ek = ((ws << 8) | h) + 1;
      uint32_t e = (ek * 0x9E3779B1u) >> 25;  // kBt2HotErr = 128
      for (int pr = 0; pr < 4; ++pr, e = (e + 1) & (kBt2HotErr - 1)) {
        uint32_t k = herr[e].x;
        if (k == 0) k = atomicCAS(&herr[e].x, 0u, ek);
        if (k == 0 || k == ek) {
          atomicAdd(&herr[e].y, 1u);
          return;
        }
      }
      Path::cold_err(kp, Path::cold_key(P, id), ws);
    }
  };
  // the overflow table: false when the id is not in it and its 8 probes are
  // taken
  auto hot_try = [&](Id id, uint64_t d, bool err, uint32_t ws) -> bool {
    uint32_t h = hot_home(id);
    for (int pr = 0; pr < 8; ++pr) {
      unsigned long long k = hkey[h];
      if (k == 0) k = atomicCAS(&hkey[h], 0ULL, (unsigned long long)id);
      if (k == 0 || k == id) {
        hot_acc(h, id, d, err, ws);
        return true;
      }
      h = h + 1 == kBt2Hot ? 0u : h + 1;
    }
    return false;
  };
  // a span its region cannot take: the overflow table, else the direct path
  auto hot_add = [&](Id id, uint64_t d, bool err, uint32_t ws) {
    if (hot_try(id, d, err, ws)) return;
    n_drop += Path::cold_direct(kp, Path::cold_key(P, id), d, bucket_lds<1>(d, lbins, P), err, ws);
  };
  auto hot_rec = [&](uint32_t b, const Rec &r) {
    hot_add(Path::rec_id(b, r), Path::rec_d(r), Path::rec_err(r), Path::rec_ws(r));
  };
  // claims n record positions of bin b's region (u16 pairs); positions at or
  // past the region's end take the overflow table instead
  auto claim = [&](uint32_t b, uint32_t n) -> uint32_t {
    const uint32_t sh = (b & 1u) * 16;
    return (atomicAdd(&rcnw[b >> 1], n << sh) >> sh) & 0xFFFFu;
  };
  auto place = [&](Id id, uint64_t d, bool err, uint32_t ws) {
    const uint32_t h0 = hot_home(id);
    const ulonglong2 hk = *reinterpret_cast<const ulonglong2 *>(hkey + h0);
    if (hk.x == id || hk.y == id) {
      hot_acc(h0 + (hk.x == id ? 0u : 1u), id, d, err, ws);
      return;
    }
    const uint32_t bk = bucket_lds<1>(d, lbins, P);
    if (__builtin_expect(d > Path::kDurMask, 0)) {  // beyond the record's duration bits: the direct path
      n_drop += Path::cold_direct(kp, Path::cold_key(P, id), d, bk, err, ws);
      return;
    }
    const uint32_t b = (uint32_t)(id >> Path::kBinLsb) & (kPartBins - 1), sh = (b & 1u) * 16;
    const uint32_t c = (atomicAdd(&fillw[b >> 1], 1u << sh) >> sh) & 0xFFFFu;
    const Rec rec = Path::rec(id, d, bk, err, ws);
    if (c < kStage) {
      stage[b * kStage + c] = rec;
      return;
    }
    // the stage is full this round.  An id that holds two or more of its
    // slots is frequent (a hot series of a skewed mix): it moves to the
    // overflow table; any other record is stored on its own.  (The slots may
    // hold this round's records or, not yet overwritten, an earlier round's:
    // either way records of this bin, which is all the test needs.)
    uint32_t same = 0;
#pragma unroll
    for (uint32_t q = 0; q < kStage; ++q) same += Path::same_id(stage[b * kStage + q], rec) ? 1u : 0u;
    // (a frequent id the full overflow table cannot take stays a record:
    // the per-span direct path is only for a region that is used up)
    if (same >= 2 && hot_try(id, d, err, ws)) return;
    const uint32_t at = claim(b, 1);
    if (at < region) my_rec[b * bin_stride + at] = rec;
    else hot_add(id, d, err, ws);
  };
  auto hll_settle = [&](const Pending<2> &q) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (((q.hv[j] >> ((q.hoff[j] & 3u) * 8)) & 0xFFu) < q.rho[j]) {
        const uint32_t slot = atomicAdd(&hq_n[0], 1u);
        if (slot < kBtHq) hq[slot] = make_uint2(q.hoff[j], q.rho[j]);
        else hll_raise(kp->hll + q.hoff[j], q.rho[j]);
      }
    }
  };

  const uint32_t hp = P.p, lbs = P.lb_shift;
  auto step = [&](SpanTile<2> &T, uint32_t toff, uint32_t pf) {
    Id id[2];
    uint64_t d[2];
    uint32_t ws[2], hoff[2], rho[2];
    bool err[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool valid = lane_off + toff + (uint32_t)j < len;
      const uint64_t key = copy_u64(T.key[j]);  // 0 past the range
      n_zero += wave_count(valid && key == 0);
      d[j] = T.e[j] > T.s[j] ? T.e[j] - T.s[j] : 0;
      const uint32_t meta = copy_u32(T.meta[j]);
      const uint32_t svc = meta & 0xFFFFu;
      const bool svc_ok = svc < P.n_services;
      ws[j] = window_slot_lean(P, T.e[j]);
      const bool win_ok = ws[j] != 0xFFFFFFFFu;
      n_badsvc += wave_count(valid && !svc_ok);
      n_oor += wave_count(valid && svc_ok && !win_ok);
      const bool sk = valid && svc_ok && win_ok;
      err[j] = sk && ((meta >> 19) & 3u) == 2u;
      // an ERROR span of no series (key 0) has no record: its count-min cells
      // here, as on every other path (key 0's cells)
      if (err[j] && key == 0) bt_err_no_series(kp, ws[j]);
      id[j] = Path::id(P, key, n_drop, cap);  // (here: earlier or later in this body moves the hashed instance's code)
      // the span hash on 32-bit halves, rho without 64-bit shifts, the
      // register row by a 24-bit multiply-add (as the lean C2 kernel)
      const H64 x = xxh64_16_h(T.a[j], T.b[j]);
      const uint32_t yh = __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - hp), yl = (x.lo << hp) | (1u << (hp - 1));
      const uint32_t r = (uint32_t)__clzll((long long)(((uint64_t)yh << 32) | yl)) + 1;
      uint32_t row;
      asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(ws[j]), "s"(P.n_services), "v"(svc));
      const uint32_t ho = sk ? (row << hp) + (x.hi >> (32 - hp)) : 0u;
      bool up = sk && !(MODE & 2);
      if (lb_on) {
        const bool f = r <= llb[ho >> lbs];
        n_filt += (up && f) ? 1u : 0u;
        up = up && !f;
      }
      rho[j] = up ? r : 0u;
      hoff[j] = up ? ho : 0u;
    }
    uint32_t hv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
      hv[j] = (MODE & 2) ? 0xFFFFFFFFu : *reinterpret_cast<const uint32_t *>(P.hll + (hoff[j] & ~3u));
    __builtin_amdgcn_sched_barrier(0);
    load_tile_at<2, 2>(P, lo + pf, tremain(pf), lane_off, T);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (MODE & 1) n_drop += (uint32_t)((id[j] ^ d[j]) == 0x123456789ABCULL);  // keep the values live
      else if (id[j] != 0) place(id[j], d[j], err[j], ws[j]);
    }
    hll_settle(pend2);
    pend2 = pend;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      pend.hoff[j] = hoff[j];
      pend.rho[j] = rho[j];
      pend.hv[j] = hv[j];
    }
  };
  // the waves write out the full stages of their 128 bins
  uint16_t *wl = flist + wave * 128;
  auto flush = [&]() {
    const uint32_t fw = fillw[threadIdx.x];  // bins 2t, 2t + 1
    const bool f0 = (fw & 0xFFFFu) >= kStage, f1 = (fw >> 16) >= kStage;
    if (f0 || f1) fillw[threadIdx.x] = (f0 ? 0u : (fw & 0xFFFFu)) | (f1 ? 0u : (fw & 0xFFFF0000u));
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
    const uint32_t n0 = (uint32_t)__popcll(m0), nf = n0 + (uint32_t)__popcll(m1);
    if (f0) wl[lane_rank(m0)] = (uint16_t)(2 * threadIdx.x);
    if (f1) wl[n0 + lane_rank(m1)] = (uint16_t)(2 * threadIdx.x + 1);
    compiler_fence();  // one wave's LDS operations complete in order
    for (uint32_t i0 = 0; i0 < nf; i0 += 64 / kStage) {  // wave-uniform
      const uint32_t i = i0 + lane / kStage, q = lane & (kStage - 1);
      const bool act = i < nf;
      const uint32_t b = act ? wl[i] : 0u;
      const Rec r = stage[b * kStage + q];
      uint32_t at = act && q == 0 ? claim(b, kStage) : 0u;
      at = (uint32_t)__shfl((int)at, (int)(lane & ~(kStage - 1)), 64);
      if (act) {
        if (MODE & 16) my_rec[(uint64_t)threadIdx.x * 64 + ((i0 + at) & 63)] = r;  // ablation: no scatter
        else if (MODE & 32) (void)0;                                          // ablation: no store
        else if (at + q < region) my_rec[b * bin_stride + at + q] = r;
        else hot_rec(b, r);
      }
    }
  };

  // Stage flushes: after every round, or -- once the first two rounds have
  // put 32 or more ids in the overflow table (a skewed mix, whose hot series
  // bypass the stages) -- after every second round, which halves the
  // barriers (for uniform keys the fuller stages would spill more records).
  bool sparse = false;  // workgroup-uniform: read from LDS after a barrier
  for (uint32_t r = 0; r < rounds; r += 2) {
    step(buf[0], tstart(r), tstart(r + 2));
    if (!sparse) {
      __syncthreads();
      if (!(MODE & 1)) flush();
      __syncthreads();
    }
    if (r + 1 < rounds) step(buf[1], tstart(r + 1), tstart(r + 3));
    __syncthreads();
    if (!(MODE & 1)) flush();
    if (r == 0 && wave == 0) {
      uint32_t used = 0;
      for (uint32_t h = lane; h < kBt2Hot; h += 64) used += wave_count(hkey[h] != 0);
      if (lane == 0) hq_n[2] = used >= 32 ? 1u : 0u;
    }
    __syncthreads();
    if (r == 0) sparse = (MODE & 64) ? true : hq_n[2] != 0;
  }
  hll_settle(pend2);
  hll_settle(pend);
  // the wave's bound sub-block, loaded now (hll_lb_pre): it lands during the
  // stage flush and the overflow table's flush below
  uint4 lbv[4];
  hll_lb_pre<kBtBlock>(P, lbv);
  stamp(2);
  // partial stages, then this workgroup's region fills
  for (uint32_t b = threadIdx.x; b < kPartBins; b += kBtBlock) {
    uint32_t c = (fillw[b >> 1] >> ((b & 1u) * 16)) & 0xFFFFu;  // < kStage after the last flush
    if constexpr (Path::kClampDrain) c = min(c, kStage);
    const uint32_t at = c ? claim(b, c) : 0u;
    for (uint32_t q = 0; q < c; ++q) {
      if (at + q < region) my_rec[b * bin_stride + at + q] = stage[b * kStage + q];
      else hot_rec(b, stage[b * kStage + q]);
    }
  }
  __syncthreads();
  // the queued HLL raises' register words, read now (the queue is final after
  // the barrier above) and CAS-raised at the end: the reads overlap the
  // overflow table's flush instead of adding a round trip
  const uint32_t nq = min(hq_n[0], kBtHq);
  constexpr uint32_t kQ = (kBtHq + kBtBlock - 1) / kBtBlock;
  uint32_t qv[kQ];
#pragma unroll
  for (uint32_t i = 0; i < kQ; ++i) {
    const uint32_t t = threadIdx.x + i * kBtBlock;
    qv[i] = t < nq ? __hip_atomic_load(reinterpret_cast<const uint32_t *>(P.hll + (hq[t].x & ~3u)), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT)
                   : 0u;
  }
  for (uint32_t b = threadIdx.x; b < kPartBins; b += kBtBlock)
    P.bt_cnt[(uint64_t)b * P.bt_grid + blockIdx.x] = min((rcnw[b >> 1] >> ((b & 1u) * 16)) & 0xFFFFu, region);
  // the overflow table.  With kLookup, first each entry's row (find-or-insert,
  // one lane per entry) into the LDS of the flush lists (the stages are all
  // out); an entry whose bin is full is dropped.
  uint32_t *hslot = reinterpret_cast<uint32_t *>(flist);  // [kBt2Hot]
  if constexpr (Path::kLookup) {
    __syncthreads();
    for (uint32_t h = threadIdx.x; h < kBt2Hot; h += kBtBlock) {
      const unsigned long long m = hkey[h];
      uint32_t s = kNotFound;
      if (m != 0) {
        s = Path::lookup(P, m);
        if (s == kNotFound)
          for (uint32_t b = 0; b < P.nbk; ++b) n_drop += (hcnt[h * kPartWords + (b >> 1)] >> ((b & 1u) * 16)) & 0xFFFFu;
      }
      hslot[h] = s;
    }
    __syncthreads();
  }
  // Then each entry's counts and ns sum added to its row's spill cells
  // (atomics: the entries of one id come from every workgroup), two entries
  // per wave instruction and one cell per lane: an entry's nbk counts and ns
  // sum are contiguous in base64, so it leaves as three 64-B atomic requests,
  // where one lane's nbk + 1 serial atomics made a Zipf mix's epilogue
  // (hundreds of hot series in every workgroup's table) the scatter's longest
  // phase
  {
    const uint32_t half = lane >> 5, cell = lane & 31u, nc = P.nbk + 1;
    static_assert(kBt2Hot % 2 == 0 && kPartMaxBk + 1 <= 32, "overflow flush geometry");
    for (uint32_t h0 = wave * 2; h0 < kBt2Hot; h0 += kWaves * 2) {
      const uint32_t h = h0 + half;
      uint32_t s;
      if constexpr (Path::kLookup) {
        s = hslot[h];
        if (s == kNotFound || cell >= nc) continue;
      } else {
        const uint32_t idx = (uint32_t)hkey[h];
        if (idx == 0 || cell >= nc) continue;
        s = Path::row(P, idx);
      }
      const unsigned long long v = cell == P.nbk ? hsum[h]
                                                 : (hcnt[h * kPartWords + (cell >> 1)] >> ((cell & 1u) * 16)) & 0xFFFFu;
      if (v) atomicAdd(P.base64 + (uint64_t)s * nc + cell, v);
    }
  }
  if (threadIdx.x < kBt2HotErr) {
    const uint2 e = herr[threadIdx.x];
    if (e.x) {
      const uint32_t ws = (e.x - 1) >> 8, h = (e.x - 1) & 0xFFu;
      if constexpr (Path::kLookup) {
        const uint32_t s = hslot[h];
        if (s != kNotFound) atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + s, (unsigned long long)e.y);
        else
          for (uint32_t i = 0; i < e.y; ++i) Path::err_no_row(kp, P, hkey[h], ws);
      } else {
        atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + Path::row(P, (uint32_t)hkey[h]), (unsigned long long)e.y);
      }
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kQ; ++i) {
    const uint32_t t = threadIdx.x + i * kBtBlock;
    if (t >= nq) continue;
    const uint2 q = hq[t];
    hll_raise_from(gbl(reinterpret_cast<uint32_t *>(P.hll + (q.x & ~3u))), qv[i], (q.x & 3u) * 8, q.y);
  }
  n_drop = wave_sum(n_drop);
  n_filt = wave_sum(n_filt);
  if (lane == 0) {
    // a slot per workgroup (same-address atomics from every wave would
    // serialise the tail of the launch)
    if (n_filt) atomicAdd(&P.hll_filt[blockIdx.x & (kFiltSlots - 1)], (unsigned long long)n_filt);
    if (n_zero) atomicAdd(&P.stats[kStatZeroKey], (unsigned long long)n_zero);
    if (n_badsvc) atomicAdd(&P.stats[kStatInvalidService], (unsigned long long)n_badsvc);
    if (n_oor) atomicAdd(&P.stats[kStatWindowOOR], (unsigned long long)n_oor);
    if (n_drop) atomicAdd(&P.stats[kStatDropped], (unsigned long long)n_drop);
  }
  hll_lb_finish<kBtBlock>(P, lbv);
  stamp(3);
}

}  // namespace
}  // namespace sa
