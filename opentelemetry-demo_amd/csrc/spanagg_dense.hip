// spanagg_dense.hip -- the dense-index form of the binned high-cardinality
// path of libspanagg (gfx950), SA_OPT_DENSE_IDS.  The host resolves every
// span's series in its own dictionary and hands the engine a small dense
// index i instead of the 64-bit series hash (sa_bind_ids declares which hash
// an index stands for), so the row of a span is arithmetic:
//   bin = i & (kPartBins - 1), in-bin slot = i >> kPartBinBits,
//   row = bin << log2sb | in-bin slot
// (low bits pick the bin: indices handed out in order fill every bin evenly
// from the first series on).  Nothing is looked up or inserted anywhere.
//
// Two kernels per launch, the shape of spanagg_binned.hip's:
//   dn_scatter_kernel (one 1,024-thread workgroup per CU, ~160 KiB LDS)
//     bt_scatter2_kernel's skeleton -- register tile ring, per-span stats,
//     HLL with the lower-bound filter, round-synchronous LDS stages per bin,
//     the LDS overflow table for hot indices, the same bt_cnt region fills --
//     with 8-B records (dn_rec) in 8-record stages that leave as aligned 64-B
//     chunks, no multiply, and cold paths (region used up, duration beyond
//     the record's bits) that add straight into base64[row] and
//     errcnt[ws][row] with atomics.
//   dn_aggregate_kernel (one 512-thread workgroup per bin)
//     u64 ns sums and packed u16 bucket counts per in-bin slot in LDS (no key
//     mirror): a record feeds its two LDS atomics and nothing else.  Then the
//     32-B row of each touched slot is read, added to and written back (one
//     owner, plain stores; a count that would pass 255 moves to base64) and
//     the ERROR list goes to errcnt.
// Rows, base64, errcnt and the key array (gkeys[row] = the bound hash, kmul =
// kinv = 1) have the binned path's layout, so the flush-time kernels serve
// both.
#include <algorithm>
#include <cstdlib>

#include "sa_device.h"

namespace sa {
namespace {

__device__ __forceinline__ void compiler_fence() { asm volatile("" ::: "memory"); }

typedef SA_CONST const IngestParams *KParams;
__device__ __forceinline__ KParams kernel_params() {
  return (KParams)__builtin_amdgcn_kernarg_segment_ptr();
}

// The 8-B record of one span in the region of (its bin, scatter workgroup):
//   bits  0-36  duration in ns (a longer span, 137 s, takes the cold path)
//   bits 37-41  histogram bucket (the scatter's bin table: the aggregate
//               needs no thresholds)
//   bits 42-52  in-bin slot (tables of up to 2^22 slots: 2,048 per bin)
//   bits 53-62  window slot (ERROR records; 0 otherwise)
//   bit  63     ERROR
constexpr uint32_t kDnDurBits = 37, kDnSlotShift = 42, kDnWsShift = 53;
constexpr uint64_t kDnDurMask = (1ULL << kDnDurBits) - 1;
static_assert(kPartMaxBk <= 32, "record bucket field");
__device__ __forceinline__ uint64_t dn_rec(uint32_t slot, uint64_t d, uint32_t bk, bool err, uint32_t ws) {
  return d | ((uint64_t)bk << kDnDurBits) | ((uint64_t)slot << kDnSlotShift) |
         (err ? (1ULL << 63) | ((uint64_t)ws << kDnWsShift) : 0ULL);
}
__device__ __forceinline__ uint32_t dn_row(uint32_t idx, uint32_t log2sb) {
  return ((idx & (kPartBins - 1)) << log2sb) | (idx >> kPartBinBits);
}

// Cold paths of the scatter: one span straight into its row's spill cells.
__device__ __noinline__ void dn_cold_direct(KParams Q, uint32_t row, uint64_t d, uint32_t bk, bool err, uint32_t ws) {
  unsigned long long *cells = Q->base64 + (uint64_t)row * (Q->nbk + 1);
  atomicAdd(cells + bk, 1ULL);
  if (d) atomicAdd(cells + Q->nbk, (unsigned long long)d);
  if (err) atomicAdd(Q->errcnt + ((uint64_t)ws << Q->log2cap) + row, 1ULL);
}
__device__ __noinline__ void dn_cold_err(KParams Q, uint32_t row, uint32_t ws) {
  atomicAdd(Q->errcnt + ((uint64_t)ws << Q->log2cap) + row, 1ULL);
}

__device__ __forceinline__ uint32_t lane_rank(uint64_t mask) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Round-synchronous scatter (see bt_scatter2_kernel for the scheme).  Every
// span with a valid index claims a slot of its bin's 8-record LDS stage; after
// a barrier each wave writes the full stages of its 128 bins out, eight lanes
// per stage, so a stage leaves as one aligned 64-B piece.  Indices already in
// the overflow table are added there; a span whose stage is full in its round
// is stored on its own (or moves to the overflow table when its index already
// holds two of the stage's slots); a span whose region is used up goes to the
// overflow table, past that to the row's spill cells by atomics.
// u16 counters: a workgroup takes at most kBtMaxWgSpans (65,520) spans per
// launch, which bounds its region claims per bin and every overflow-table
// count.
__global__ __launch_bounds__(kBtBlock) void dn_scatter_kernel(IngestParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t kWaves = kBtBlock / 64;
  unsigned long long *stage = reinterpret_cast<unsigned long long *>(smem);          // [bins][8]
  uint32_t *fillw = reinterpret_cast<uint32_t *>(stage + kPartBins * kDnStage);      // [bins / 2] u16 pairs
  uint32_t *rcnw = fillw + kPartBins / 2;                                            // [bins / 2] region fills
  uint16_t *flist = reinterpret_cast<uint16_t *>(rcnw + kPartBins / 2);              // [waves][128]
  unsigned long long *hkey = reinterpret_cast<unsigned long long *>(flist + kWaves * 128);  // the entry's index
  unsigned long long *hsum = hkey + kBt2Hot;
  uint32_t *hcnt = reinterpret_cast<uint32_t *>(hsum + kBt2Hot);  // [kBt2Hot][kPartWords] u16 pairs
  uint2 *hq = reinterpret_cast<uint2 *>(hcnt + kBt2Hot * kPartWords);
  uint32_t *hq_n = reinterpret_cast<uint32_t *>(hq + kBtHq);
  BinEntry *lbins = reinterpret_cast<BinEntry *>(hq_n + 4);
  uint2 *herr = reinterpret_cast<uint2 *>(lbins + kBins);  // [kBt2HotErr] {(ws << 8 | entry) + 1, count}
  uint8_t *llb = reinterpret_cast<uint8_t *>(herr + kBt2HotErr);
  const KParams kp = kernel_params();

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
  const uint32_t lb_on = P.lb_n != 0;
  uint32_t lbw = 0;
  if (lb_on && threadIdx.x * 4 < P.lb_n) lbw = *reinterpret_cast<const uint32_t *>(P.hll_lb + threadIdx.x * 4);
  SpanTile<2> buf[2];
  Pending<2> pend, pend2;  // HLL reads of the last two rounds (compared two rounds later)
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

  uint32_t n_zero = 0, n_badsvc = 0, n_oor = 0;  // wave-uniform (SGPR)
  uint32_t n_drop = 0;                           // per lane: indices at or past the table's capacity
  uint32_t n_filt = 0;                           // per lane: HLL updates the lower-bound filter skipped
#pragma unroll
  for (int j = 0; j < 2; ++j) pend.hoff[j] = pend.rho[j] = pend2.hoff[j] = pend2.rho[j] = 0;
  const uint32_t region = P.bt_region, log2sb = P.log2sb;
  unsigned long long *my_rec = reinterpret_cast<unsigned long long *>(P.bt_rec) + (uint64_t)blockIdx.x * region;
  const uint64_t bin_stride = (uint64_t)P.bt_grid * region;  // + bin * grid * region
  const uint64_t cap = 1ULL << P.log2cap;

  // overflow-table home: an even entry, probed as a pair first
  auto hot_home = [&](uint32_t idx) -> uint32_t {
    return (uint32_t)(((uint64_t)(idx * 0x9E3779B1u) * (kBt2Hot / 2)) >> 32) * 2;
  };
  auto hot_acc = [&](uint32_t h, uint32_t idx, uint64_t d, bool err, uint32_t ws) {
    const uint32_t bk = bucket_lds<1>(d, lbins, P);
    atomicAdd(&hcnt[h * kPartWords + (bk >> 1)], 1u << ((bk & 1u) * 16));
    atomicAdd(&hsum[h], (unsigned long long)d);
    if (err) {  // ERROR count per (window slot, entry); a full table adds to errcnt directly
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
      dn_cold_err(kp, dn_row(idx, log2sb), ws);
    }
  };
  // the overflow table: false when the index is not in it and its 8 probes
  // are taken
  auto hot_try = [&](uint32_t idx, uint64_t d, bool err, uint32_t ws) -> bool {
    uint32_t h = hot_home(idx);
    for (int pr = 0; pr < 8; ++pr) {
      unsigned long long k = hkey[h];
      if (k == 0) k = atomicCAS(&hkey[h], 0ULL, (unsigned long long)idx);
      if (k == 0 || k == idx) {
        hot_acc(h, idx, d, err, ws);
        return true;
      }
      h = h + 1 == kBt2Hot ? 0u : h + 1;
    }
    return false;
  };
  // a span its region cannot take: the overflow table, else its row's spill cells
  auto hot_add = [&](uint32_t idx, uint64_t d, bool err, uint32_t ws) {
    if (hot_try(idx, d, err, ws)) return;
    dn_cold_direct(kp, dn_row(idx, log2sb), d, bucket_lds<1>(d, lbins, P), err, ws);
  };
  auto hot_rec = [&](uint32_t b, unsigned long long r) {
    const uint32_t idx = ((uint32_t)(r >> kDnSlotShift) & (kPartBins - 1)) << kPartBinBits | b;
    hot_add(idx, r & kDnDurMask, (r >> 63) != 0, (uint32_t)(r >> kDnWsShift) & 1023u);
  };
  // claims n record positions of bin b's region (u16 pairs); positions at or
  // past the region's end take the overflow table instead
  auto claim = [&](uint32_t b, uint32_t n) -> uint32_t {
    const uint32_t sh = (b & 1u) * 16;
    return (atomicAdd(&rcnw[b >> 1], n << sh) >> sh) & 0xFFFFu;
  };
  static_assert(kPartBinBits == 11, "the record's slot field and hot_rec take 11-bit in-bin slots");
  auto place = [&](uint32_t idx, uint64_t d, bool err, uint32_t ws) {
    const uint32_t h0 = hot_home(idx);
    const ulonglong2 hk = *reinterpret_cast<const ulonglong2 *>(hkey + h0);
    if (hk.x == idx || hk.y == idx) {
      hot_acc(h0 + (hk.x == idx ? 0u : 1u), idx, d, err, ws);
      return;
    }
    const uint32_t bk = bucket_lds<1>(d, lbins, P);
    if (__builtin_expect(d > kDnDurMask, 0)) {  // beyond the record's duration bits
      dn_cold_direct(kp, dn_row(idx, log2sb), d, bk, err, ws);
      return;
    }
    const uint32_t b = idx & (kPartBins - 1), sh = (b & 1u) * 16;
    const uint32_t c = (atomicAdd(&fillw[b >> 1], 1u << sh) >> sh) & 0xFFFFu;
    const unsigned long long rec = dn_rec(idx >> kPartBinBits, d, bk, err, ws);
    if (c < kDnStage) {
      stage[b * kDnStage + c] = rec;
      return;
    }
    // the stage is full this round: an index that holds two or more of its
    // slots is frequent and moves to the overflow table; any other record is
    // stored on its own.  (The slots may hold an earlier round's records:
    // records of this bin either way.)
    uint32_t same = 0;
#pragma unroll
    for (uint32_t q = 0; q < kDnStage; ++q)
      same += (((stage[b * kDnStage + q] ^ rec) >> kDnSlotShift) & (kPartBins - 1)) == 0 ? 1u : 0u;
    if (same >= 2 && hot_try(idx, d, err, ws)) return;
    const uint32_t at = claim(b, 1);
    if (at < region) my_rec[b * bin_stride + at] = rec;
    else hot_add(idx, d, err, ws);
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
    uint64_t d[2];
    uint32_t idx[2], ws[2], hoff[2], rho[2];
    bool err[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const bool valid = lane_off + toff + (uint32_t)j < len;
      const uint64_t key = copy_u64(T.key[j]);  // 0 past the range
      n_zero += wave_count(valid && key == 0);
      // an index at or past the table's capacity: counted dropped, no record
      // (its HLL register is still raised below, as a key-0 span's)
      const bool big = key >= cap;
      n_drop += big ? 1u : 0u;
      idx[j] = big ? 0u : (uint32_t)key;
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
      const H64 x = xxh64_16_h(T.a[j], T.b[j]);
      const uint32_t yh = __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - hp), yl = (x.lo << hp) | (1u << (hp - 1));
      const uint32_t r = (uint32_t)__clzll((long long)(((uint64_t)yh << 32) | yl)) + 1;
      uint32_t row;
      asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(row) : "v"(ws[j]), "s"(P.n_services), "v"(svc));
      const uint32_t ho = sk ? (row << hp) + (x.hi >> (32 - hp)) : 0u;
      bool up = sk;
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
    for (int j = 0; j < 2; ++j) hv[j] = *reinterpret_cast<const uint32_t *>(P.hll + (hoff[j] & ~3u));
    __builtin_amdgcn_sched_barrier(0);
    load_tile_at<2, 2>(P, lo + pf, tremain(pf), lane_off, T);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      if (idx[j] != 0) place(idx[j], d[j], err[j], ws[j]);
    hll_settle(pend2);
    pend2 = pend;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      pend.hoff[j] = hoff[j];
      pend.rho[j] = rho[j];
      pend.hv[j] = hv[j];
    }
  };
  // the waves write out the full stages of their 128 bins (8 lanes a stage)
  uint16_t *wl = flist + wave * 128;
  auto flush = [&]() {
    const uint32_t fw = fillw[threadIdx.x];  // bins 2t, 2t + 1
    const bool f0 = (fw & 0xFFFFu) >= kDnStage, f1 = (fw >> 16) >= kDnStage;
    if (f0 || f1) fillw[threadIdx.x] = (f0 ? 0u : (fw & 0xFFFFu)) | (f1 ? 0u : (fw & 0xFFFF0000u));
    const uint64_t m0 = __ballot(f0), m1 = __ballot(f1);
    const uint32_t n0 = (uint32_t)__popcll(m0), nf = n0 + (uint32_t)__popcll(m1);
    if (f0) wl[lane_rank(m0)] = (uint16_t)(2 * threadIdx.x);
    if (f1) wl[n0 + lane_rank(m1)] = (uint16_t)(2 * threadIdx.x + 1);
    compiler_fence();  // one wave's LDS operations complete in order
    for (uint32_t i0 = 0; i0 < nf; i0 += 64 / kDnStage) {  // wave-uniform
      const uint32_t i = i0 + lane / kDnStage, q = lane & (kDnStage - 1);
      const bool act = i < nf;
      const uint32_t b = act ? wl[i] : 0u;
      const unsigned long long r = stage[b * kDnStage + q];
      uint32_t at = act && q == 0 ? claim(b, kDnStage) : 0u;
      at = (uint32_t)__shfl((int)at, (int)(lane & ~(kDnStage - 1)), 64);
      if (act) {
        if (at + q < region) my_rec[b * bin_stride + at + q] = r;
        else hot_rec(b, r);
      }
    }
  };

  // Stage flushes: after every round, or -- once the first two rounds have
  // put 32 or more indices in the overflow table (a skewed mix, whose hot
  // indices bypass the stages) -- after every second round.
  bool sparse = false;  // workgroup-uniform: read from LDS after a barrier
  for (uint32_t r = 0; r < rounds; r += 2) {
    step(buf[0], tstart(r), tstart(r + 2));
    if (!sparse) {
      __syncthreads();
      flush();
      __syncthreads();
    }
    if (r + 1 < rounds) step(buf[1], tstart(r + 1), tstart(r + 3));
    __syncthreads();
    flush();
    if (r == 0 && wave == 0) {
      uint32_t used = 0;
      for (uint32_t h = lane; h < kBt2Hot; h += 64) used += wave_count(hkey[h] != 0);
      if (lane == 0) hq_n[2] = used >= 32 ? 1u : 0u;
    }
    __syncthreads();
    if (r == 0) sparse = hq_n[2] != 0;
  }
  hll_settle(pend2);
  hll_settle(pend);
  uint4 lbv[4];
  hll_lb_pre<kBtBlock>(P, lbv);
  // partial stages, then this workgroup's region fills
  for (uint32_t b = threadIdx.x; b < kPartBins; b += kBtBlock) {
    const uint32_t c = min((fillw[b >> 1] >> ((b & 1u) * 16)) & 0xFFFFu, kDnStage);  // < kDnStage after a flush
    const uint32_t at = c ? claim(b, c) : 0u;
    for (uint32_t q = 0; q < c; ++q) {
      if (at + q < region) my_rec[b * bin_stride + at + q] = stage[b * kDnStage + q];
      else hot_rec(b, stage[b * kDnStage + q]);
    }
  }
  __syncthreads();
  // the queued HLL raises' register words, read now and CAS-raised at the end
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
  // the overflow table: each entry's counts and ns sum added to its row's
  // spill cells (atomics: the entries of one index come from every
  // workgroup), two entries per wave instruction and one cell per lane
  {
    const uint32_t half = lane >> 5, cell = lane & 31u, nc = P.nbk + 1;
    static_assert(kBt2Hot % 2 == 0 && kPartMaxBk + 1 <= 32, "overflow flush geometry");
    for (uint32_t h0 = wave * 2; h0 < kBt2Hot; h0 += kWaves * 2) {
      const uint32_t h = h0 + half;
      const uint32_t idx = (uint32_t)hkey[h];
      if (idx == 0 || cell >= nc) continue;
      const unsigned long long v = cell == P.nbk ? hsum[h]
                                                 : (hcnt[h * kPartWords + (cell >> 1)] >> ((cell & 1u) * 16)) & 0xFFFFu;
      if (v) atomicAdd(P.base64 + (uint64_t)dn_row(idx, log2sb) * nc + cell, v);
    }
  }
  if (threadIdx.x < kBt2HotErr) {
    const uint2 e = herr[threadIdx.x];
    if (e.x) {
      const uint32_t ws = (e.x - 1) >> 8, h = (e.x - 1) & 0xFFu;
      const uint32_t idx = (uint32_t)hkey[h];
      atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + dn_row(idx, log2sb), (unsigned long long)e.y);
    }
  }
#pragma unroll
  for (uint32_t i = 0; i < kQ; ++i) {
    const uint32_t t = threadIdx.x + i * kBtBlock;
    if (t >= nq) continue;
    const uint2 q = hq[t];
    SA_GLOBAL uint32_t *word = gbl(reinterpret_cast<uint32_t *>(P.hll + (q.x & ~3u)));
    const uint32_t sh = (q.x & 3u) * 8;
    uint32_t old = qv[i];
    while (((old >> sh) & 0xFFu) < q.y) {  // a failed CAS refreshes `old`
      const uint32_t nw = (old & ~(0xFFu << sh)) | (q.y << sh);
      if (__hip_atomic_compare_exchange_strong(word, &old, nw, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        break;
    }
  }
  n_drop = wave_sum(n_drop);
  n_filt = wave_sum(n_filt);
  if (lane == 0) {
    if (n_filt) atomicAdd(&P.hll_filt[blockIdx.x & (kFiltSlots - 1)], (unsigned long long)n_filt);
    if (n_zero) atomicAdd(&P.stats[kStatZeroKey], (unsigned long long)n_zero);
    if (n_badsvc) atomicAdd(&P.stats[kStatInvalidService], (unsigned long long)n_badsvc);
    if (n_oor) atomicAdd(&P.stats[kStatWindowOOR], (unsigned long long)n_oor);
    if (n_drop) atomicAdd(&P.stats[kStatDropped], (unsigned long long)n_drop);
  }
  hll_lb_finish<kBtBlock>(P, lbv);
}

// Aggregate.  One 512-thread workgroup per bin; its LDS holds, per in-bin
// slot, the u64 ns sum and 17 packed u16 bucket counts, then the ERROR list
// and the region fills (86 KiB at 2,048 slots).  Each wave instruction reads
// two regions (lanes 0-31 and 32-63, one record per lane); a wave takes every
// eighth region pair and issues four pairs' loads before it aggregates them.
// u16 counters cannot wrap: a slot's count is at most the bin's records of
// the launch's one or two record sets, 2 sets x bt_grid regions x bt_region
// records -- the engine creates a dense engine only when that, at the largest
// launch (kBtMaxWgSpans spans per scatter workgroup: 64-record regions, 256
// workgroups on an MI355X: 32,768), stays below 65,536 (dn_counters_fit); the
// scatter's overflow table and cold paths add to base64, never here.
constexpr uint32_t kDnAggBlock = 512;
constexpr uint32_t kDnErrL = 256;  // u32 words of the ERROR list: [0] count, [1..] ws << log2sb | slot
__host__ __device__ inline uint32_t dn_cnt_words(uint32_t sb) { return (sb * kPartMaxBk + 1) / 2; }
__host__ __device__ inline uint32_t dn_off_err(uint32_t sb) { return (sb * 8 + dn_cnt_words(sb) * 4 + 7) & ~7u; }
__host__ __device__ inline uint32_t dn_off_reg(uint32_t sb) { return dn_off_err(sb) + kDnErrL * 4; }

__global__ __launch_bounds__(kDnAggBlock) void dn_aggregate_kernel(IngestParams P) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr uint32_t BLOCK = kDnAggBlock, kWaves = BLOCK / 64;
  const uint32_t log2sb = P.log2sb, sb = 1u << log2sb;
  // record sets: one, or two (P.bt_rec2: two launches' scatters aggregated
  // together, so the bin's setup and row write-back serve both)
  const uint32_t nrs = cold_params().bt_rec2 ? 2u : 1u;
  const uint32_t bin = blockIdx.x;
  unsigned long long *lsum = reinterpret_cast<unsigned long long *>(smem);
  uint32_t *lcnt = reinterpret_cast<uint32_t *>(lsum + sb);  // u16 [sb][17], packed
  uint32_t *errl = reinterpret_cast<uint32_t *>(smem + dn_off_err(sb));
  uint32_t *rcnt = reinterpret_cast<uint32_t *>(smem + dn_off_reg(sb));  // [G] region fills (the set's)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t row0 = bin << log2sb;

  // 1. region fills, zeroed counters
  for (uint32_t g = tid; g < P.bt_grid; g += BLOCK) rcnt[g] = P.bt_cnt[(uint64_t)bin * P.bt_grid + g];
  for (uint32_t s = tid; s < sb; s += BLOCK) lsum[s] = 0;
  const uint32_t cw = dn_cnt_words(sb);
  for (uint32_t i = tid; i < cw; i += BLOCK) lcnt[i] = 0;
  if (tid == 0) errl[0] = 0;
  __syncthreads();

  // 2. the records, set by set: a record feeds its two LDS atomics
  const uint32_t half = lane >> 5, r0 = lane & 31u;
  auto agg = [&](uint32_t vlo, uint32_t vhi) {
    const uint32_t s = (vhi >> (kDnSlotShift - 32)) & (sb - 1);
    uint32_t h;  // the (slot, bucket) u16 counter: s * 17 + bucket
    asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(h) : "v"(s), "i"(kPartMaxBk), "v"((vhi >> (kDnDurBits - 32)) & 31u));
    atomicAdd(&lcnt[h >> 1], 1u << ((h & 1u) << 4));
    atomicAdd(&lsum[s], ((unsigned long long)(vhi & ((1u << (kDnDurBits - 32)) - 1)) << 32) | vlo);
    if ((int32_t)vhi < 0) {
      const uint32_t ws = (vhi >> (kDnWsShift - 32)) & 1023u;
      const uint32_t at = atomicAdd(&errl[0], 1u);
      if (at + 1 < kDnErrL) errl[at + 1] = (ws << log2sb) | s;
      else dn_cold_err(kernel_params(), row0 | s, ws);  // past the LDS list
    }
  };
#pragma unroll 1
  for (uint32_t rs = 0; rs < nrs; ++rs) {
    SA_CONST const IngestParams &Q = cold_params();
    const uint32_t G = rs ? Q.bt_grid2 : P.bt_grid, region = rs ? Q.bt_region2 : P.bt_region;
    if (rs) {  // the second set's region fills (every wave is past the first set's records)
      __syncthreads();
      for (uint32_t g = tid; g < G; g += BLOCK) rcnt[g] = Q.bt_cnt2[(uint64_t)bin * G + g];
      __syncthreads();
    }
    const unsigned long long *bin_rec =
        reinterpret_cast<const unsigned long long *>(rs ? Q.bt_rec2 : P.bt_rec) + (uint64_t)bin * G * region;
    const __amdgpu_buffer_rsrc_t rrec = rsrc(bin_rec, G * region * 8);
    const uint32_t pairs = (G + 1) / 2;
    constexpr uint32_t kBatch = 4;
#pragma unroll 1
    for (uint32_t p0 = wave; p0 < pairs; p0 += kWaves * kBatch) {
      uint32_t vlo[kBatch], vhi[kBatch];
      bool ok[kBatch];
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b) {
        const uint32_t g = 2 * (p0 + b * kWaves) + half;
        const uint32_t c = rcnt[g < G ? g : 0u];
        ok[b] = g < G && r0 < c;
        // (an offset past the descriptor's range loads zeros)
        const auto x = __builtin_amdgcn_raw_buffer_load_b64(rrec, (int)(ok[b] ? (g * region + r0) * 8 : 0xFFFFFFF8u), 0, 2);
        vlo[b] = x[0];
        vhi[b] = x[1];
      }
#pragma unroll
      for (uint32_t b = 0; b < kBatch; ++b)
        if (ok[b]) agg(vlo[b], vhi[b]);
    }
    // regions longer than 32 records: the rest, one record per lane
#pragma unroll 1
    for (uint32_t p = wave; p < pairs; p += kWaves) {
      const uint32_t g = 2 * p + half;
      const uint32_t c = g < G ? min(rcnt[g], region) : 0u;
      for (uint32_t r = 32 + r0; r < c; r += 32) {
        const unsigned long long v = bin_rec[(uint64_t)g * region + r];
        agg((uint32_t)v, (uint32_t)(v >> 32));
      }
    }
  }
  __syncthreads();

  // 3. touched rows of the bin (one owner: plain stores; the scatter and the
  //    spill below add to base64 with atomics), then the ERROR list
  const uint32_t nbk = P.nbk;
  uint4 *rows = reinterpret_cast<uint4 *>(P.gcounts) + (uint64_t)row0 * (kRowBytes / 16);
  for (uint32_t s = tid; s < sb; s += BLOCK) {
    const unsigned long long ls = lsum[s];
    uint32_t a[kPartMaxBk], any = 0;
#pragma unroll
    for (uint32_t b = 0; b < kPartMaxBk; ++b) {
      const uint32_t h = s * kPartMaxBk + b;
      a[b] = b < nbk ? (lcnt[h >> 1] >> ((h & 1u) * 16)) & 0xFFFFu : 0u;
      any |= a[b];
    }
    if (!ls && !any) continue;
    const uint4 ra = rows[(uint64_t)s * 2], rb = rows[(uint64_t)s * 2 + 1];
    const uint32_t w[8] = {ra.x, ra.y, ra.z, ra.w, rb.x, rb.y, rb.z, rb.w};
    const unsigned long long sum = ((unsigned long long)w[1] << 32 | w[0]) + ls;
    uint32_t c[kPartMaxBk];
    bool spill = false;
#pragma unroll
    for (uint32_t b = 0; b < kPartMaxBk; ++b) {
      c[b] = ((w[2 + b / 4] >> ((b & 3u) * 8)) & 0xFFu) + a[b];
      spill |= c[b] > 0xFFu;
    }
    uint32_t o[6] = {0, 0, 0, 0, 0, 0};
    if (spill) {  // the row's counts move to the spill array
      unsigned long long *sp = P.base64 + (uint64_t)(row0 | s) * (nbk + 1);
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
  const uint32_t ne = min(errl[0], kDnErrL - 1);
  for (uint32_t i = tid; i < ne; i += BLOCK) {
    const uint32_t ek = errl[i + 1], ws = ek >> log2sb, s = ek & (sb - 1);
    atomicAdd(P.errcnt + ((uint64_t)ws << P.log2cap) + (row0 | s), 1ULL);
  }
}

// gkeys[row of index[j]] = key_hash[j] (sa_bind_ids; the host validated both)
__global__ void dn_bind_kernel(unsigned long long *gkeys, const uint64_t *index, const uint64_t *key_hash, uint64_t n,
                               uint32_t log2sb) {
  for (uint64_t j = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; j < n; j += (uint64_t)gridDim.x * blockDim.x)
    gkeys[dn_row((uint32_t)index[j], log2sb)] = key_hash[j];
}

}  // namespace

size_t dn_agg_lds_bytes(uint32_t log2sb, uint32_t grid) { return dn_off_reg(1u << log2sb) + (size_t)grid * 4 + 16; }

hipError_t prepare_ingest_dn(size_t agg_lds) {
  if (hipError_t e = hipFuncSetAttribute((const void *)&dn_scatter_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kBt2ScatterLds);
      e != hipSuccess)
    return e;
  return hipFuncSetAttribute((const void *)&dn_aggregate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)agg_lds);
}

hipError_t launch_dn_scatter(const IngestParams &P, hipStream_t s) {
  void *args[] = {const_cast<IngestParams *>(&P)};
  return hipLaunchKernel((const void *)&dn_scatter_kernel, dim3(P.bt_grid), dim3(kBtBlock), args, kBt2ScatterLds, s);
}

hipError_t launch_dn_aggregate(const IngestParams &P, hipStream_t s) {
  void *args[] = {const_cast<IngestParams *>(&P)};
  // (two record sets: the region-fill array holds the larger set's)
  const uint32_t g = P.bt_rec2 && P.bt_grid2 > P.bt_grid ? P.bt_grid2 : P.bt_grid;
  return hipLaunchKernel((const void *)&dn_aggregate_kernel, dim3(kPartBins), dim3(kDnAggBlock), args,
                         dn_agg_lds_bytes(P.log2sb, g), s);
}

hipError_t launch_dn_bind(unsigned long long *gkeys, const uint64_t *index, const uint64_t *key_hash, uint64_t n,
                          uint32_t log2sb, hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t block = 256;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + block - 1) / block, 1024);
  hipLaunchKernelGGL(dn_bind_kernel, dim3(grid), dim3(block), 0, s, gkeys, index, key_hash, n, log2sb);
  return hipGetLastError();
}

}  // namespace sa
