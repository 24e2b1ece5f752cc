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
//   bt_scatter2_kernel<BtDense> (one 1,024-thread workgroup per CU, ~160 KiB
//   LDS; the binned path's scatter template, sa_bt_scatter.h, with BtDense
//   below as its Path)
//     register tile ring, per-span stats, HLL with the lower-bound filter,
//     round-synchronous LDS stages per bin, the LDS overflow table for hot
//     indices and the bt_cnt region fills are the template's; BtDense gives it
//     8-B records (dn_rec) in 8-record stages that leave as aligned 64-B
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

#include "sa_bt_scatter.h"

namespace sa {
namespace {

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

// The scatter's Path (sa_bt_scatter.h) for series given by dense index.  The
// id is the index itself (0 has no record; one at or past the table's
// capacity is counted as dropped and has none either -- its HLL register is
// still raised, as a key-0 span's); a record is the 8 B of dn_rec, in
// 8-record stages.  A span past the overflow table adds straight into its
// row's spill cells, and the epilogue needs no lookup: an entry's row is
// dn_row of its index.
struct BtDense {
  typedef uint32_t Id;
  typedef unsigned long long Rec;
  static constexpr uint32_t kStage = kDnStage;
  static constexpr uint64_t kDurMask = kDnDurMask;
  static constexpr uint32_t kBinLsb = 0;
  static constexpr bool kStamps = false, kLookup = false, kClampDrain = true;
  static_assert(kPartBinBits == 11, "the record's slot field and rec_id take 11-bit in-bin slots");
  static __device__ __forceinline__ Id id(const IngestParams &, uint64_t key, uint32_t &n_drop, uint64_t cap) {
    const bool big = key >= cap;
    n_drop += big ? 1u : 0u;
    return big ? 0u : (uint32_t)key;
  }
  static __device__ __forceinline__ uint32_t home_hash(Id idx) { return idx * 0x9E3779B1u; }
  static __device__ __forceinline__ uint32_t row(const IngestParams &P, Id idx) { return dn_row(idx, P.log2sb); }
  static __device__ __forceinline__ Rec rec(Id idx, uint64_t d, uint32_t bk, bool err, uint32_t ws) {
    return dn_rec(idx >> kPartBinBits, d, bk, err, ws);
  }
  static __device__ __forceinline__ Id rec_id(uint32_t b, Rec r) {
    return ((uint32_t)(r >> kDnSlotShift) & (kPartBins - 1)) << kPartBinBits | b;
  }
  static __device__ __forceinline__ uint64_t rec_d(Rec r) { return r & kDnDurMask; }
  static __device__ __forceinline__ bool rec_err(Rec r) { return (r >> 63) != 0; }
  static __device__ __forceinline__ uint32_t rec_ws(Rec r) { return (uint32_t)(r >> kDnWsShift) & 1023u; }
  static __device__ __forceinline__ bool same_id(Rec a, Rec b) {
    return (((a ^ b) >> kDnSlotShift) & (kPartBins - 1)) == 0;
  }
  // the cold paths take the row
  static __device__ __forceinline__ uint32_t cold_key(const IngestParams &P, Id idx) { return row(P, idx); }
  static __device__ __forceinline__ uint32_t cold_direct(KParams kp, uint32_t row, uint64_t d, uint32_t bk, bool err,
                                                         uint32_t ws) {
    dn_cold_direct(kp, row, d, bk, err, ws);
    return 0u;  // never dropped
  }
  static __device__ __forceinline__ void cold_err(KParams kp, uint32_t row, uint32_t ws) { dn_cold_err(kp, row, ws); }
};

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
  if (hipError_t e = hipFuncSetAttribute((const void *)&bt_scatter2_kernel<BtDense, 0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                         (int)kBt2ScatterLds);
      e != hipSuccess)
    return e;
  return hipFuncSetAttribute((const void *)&dn_aggregate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)agg_lds);
}

hipError_t launch_dn_scatter(const IngestParams &P, hipStream_t s) {
  void *args[] = {const_cast<IngestParams *>(&P)};
  return hipLaunchKernel((const void *)&bt_scatter2_kernel<BtDense, 0>, dim3(P.bt_grid), dim3(kBtBlock), args, kBt2ScatterLds, s);
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
