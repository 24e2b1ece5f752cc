// spanagg_table.hip -- the flush-time table kernels of libspanagg: slab and
// ERROR-slab reduce, compact, dense gather, count-min fold, key count.
#include "sa_device.h"

namespace sa {
namespace {

// ---------------------------------------------------------------------------
// Flush-time kernels.
// slabs -> counters.  blockIdx.y takes a group of kSlabGroup workgroup slabs;
// each thread sums one 4-cell quad of them and adds the partial into the u64
// counters (coalesced no-return atomics, G / kSlabGroup per cell).  The slabs
// are cleared by a memset afterwards.
constexpr uint32_t kSlabGroup = 16;
__global__ void reduce_slabs_kernel(const uint32_t *slab_cnt, const unsigned long long *slab_sum,
                                    unsigned long long *gcounts, uint32_t G, uint64_t cap,
                                    uint32_t nbk) {
  const uint32_t srow = (nbk + 1) & ~1u;  // 2 * ceil(nbk / 2)
  const uint64_t cells = cap * srow, quads = cells / 4;
  const uint32_t stride = row_stride(nbk);
  const uint32_t g0 = blockIdx.y * kSlabGroup, g1 = min(G, g0 + kSlabGroup);
  const uint64_t q = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (q < quads) {
    unsigned long long acc[4] = {0, 0, 0, 0};
    for (uint32_t g = g0; g < g1; ++g) {
      const uint4 v = reinterpret_cast<const uint4 *>(slab_cnt + (uint64_t)g * cells)[q];
      acc[0] += v.x;
      acc[1] += v.y;
      acc[2] += v.z;
      acc[3] += v.w;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint64_t c = q * 4 + i, slot = c / srow, b = c - slot * srow;
      if (acc[i] && b < nbk) atomicAdd(gcounts + slot * stride + row_count_cell((uint32_t)b), acc[i]);
    }
  } else if (q < quads + cap) {
    const uint64_t slot = q - quads;
    unsigned long long acc = 0;
    for (uint32_t g = g0; g < g1; ++g) acc += slab_sum[(uint64_t)g * cap + slot];
    if (acc) atomicAdd(gcounts + slot * stride + row_sum_cell(0), acc);
  }
}

// One counter row in the external layout [nbk bucket counts, ns sum] (u64),
// from either row layout (u64 segment rows, or the binned path's 32-B u8 rows
// + the u64 spill array).
__device__ __forceinline__ bool row_nonzero(const unsigned long long *gcounts, uint64_t s, const RowGeom &g) {
  if (g.row8) {
    const uint4 *row = reinterpret_cast<const uint4 *>(gcounts) + s * (kRowBytes / 16);
    const uint4 a = row[0], b = row[1];
    if (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) return true;
    for (uint32_t c = 0; c <= g.nbk; ++c)
      if (g.base64[s * (g.nbk + 1) + c]) return true;
    return false;
  }
  const uint32_t stride = row_stride(g.nbk);
  const unsigned long long *row = gcounts + s * stride;
  for (uint32_t c = 0; c < stride; ++c)
    if (row[c]) return true;
  return false;
}

__device__ __forceinline__ void row_emit(const unsigned long long *gcounts, uint64_t s, const RowGeom &g,
                                         unsigned long long *out) {
  const uint32_t nbk = g.nbk;
  if (g.row8) {
    const unsigned long long *row = gcounts + s * (kRowBytes / 8);
    const uint8_t *cnt = reinterpret_cast<const uint8_t *>(row + 1);
    const unsigned long long *b64 = g.base64 + s * (nbk + 1);
    for (uint32_t b = 0; b < nbk; ++b) out[b] = cnt[b] + b64[b];
    out[nbk] = row[0] + b64[nbk];
    return;
  }
  const uint32_t stride = row_stride(nbk);
  const unsigned long long *row = gcounts + s * stride;
  unsigned long long sum = 0;
  for (uint32_t c = 0; c < stride; c += 8) sum += row[c];
  for (uint32_t b = 0; b < nbk; ++b) out[b] = row[row_count_cell(b)];
  out[nbk] = sum;
}

__device__ __forceinline__ void row_zero(unsigned long long *gcounts, uint64_t s, const RowGeom &g) {
  if (g.row8) {
    uint4 *row = reinterpret_cast<uint4 *>(gcounts) + s * (kRowBytes / 16);
    row[0] = row[1] = make_uint4(0, 0, 0, 0);
    for (uint32_t c = 0; c <= g.nbk; ++c) g.base64[s * (g.nbk + 1) + c] = 0;
    return;
  }
  const uint32_t stride = row_stride(g.nbk);
  for (uint32_t c = 0; c < stride; ++c) gcounts[s * stride + c] = 0;
}

// Compacts occupied slots with a non-zero row into (out_keys, out_rows); order
// is arrival order of the atomic ticket (the host sorts by key).  Keys leave
// as the host's series ids (stored id * kinv), rows in the external layout.
__global__ void compact_kernel(const unsigned long long *gkeys, unsigned long long *gcounts,
                               uint64_t cap, RowGeom g, unsigned long long *out_keys,
                               unsigned long long *out_rows, unsigned long long *out_n,
                               uint64_t out_cap, int reset) {
  const uint32_t ostride = g.nbk + 1;
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < cap;
       s += (uint64_t)gridDim.x * blockDim.x) {
    const unsigned long long k = gkeys[s];
    if (!k) {
      // dense-index engines: spans on an index that was never bound -- no
      // row is reported; a resetting pass counts them dropped and clears them
      if (g.dense && reset && row_nonzero(gcounts, s, g)) {
        const uint8_t *cnt = reinterpret_cast<const uint8_t *>(gcounts + s * (kRowBytes / 8) + 1);  // (row8)
        unsigned long long calls = 0;
        for (uint32_t b = 0; b < g.nbk; ++b) calls += cnt[b] + g.base64[s * (g.nbk + 1) + b];
        atomicAdd(g.dropped, calls);
        row_zero(gcounts, s, g);
      }
      continue;
    }
    if (!row_nonzero(gcounts, s, g)) continue;
    // one returning atomic per wave for its emitting lanes (a million lanes
    // on one counter serialised the compaction of a 1 M-series table)
    const uint64_t m = __ballot(true);
    const int leader = __builtin_ctzll(m);
    unsigned long long base = 0;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(out_n, (unsigned long long)__popcll(m));
    base = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(base >> 32), leader) << 32) |
           (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)base, leader);
    const unsigned long long pos =
        base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
    if (pos < out_cap) {
      if (out_keys) out_keys[pos] = k * g.kinv;
      if (out_rows) row_emit(gcounts, s, g, out_rows + pos * ostride);
    }
    if (reset) row_zero(gcounts, s, g);
  }
}

__device__ __forceinline__ uint32_t geom_find(const unsigned long long *gkeys, uint64_t m, const RowGeom &g) {
  if (g.binned) {
    const BtSeq q = bt_seq(m, g.log2sb);
    const uint32_t base = (uint32_t)(m >> kBinShift) << g.log2sb;
    for (uint32_t i = 0; i < bt_probe_max(g.log2sb); ++i) {
      const uint32_t s = base | bt_pos(q, i);
      const unsigned long long k = gkeys[s];
      if (k == m) return s;
      if (k == 0) return kNotFound;
    }
    return kNotFound;
  }
  return g_find(gkeys, m, g.log2cap, g.max_probe);
}

// rows[i] = [nbk bucket counts, ns sum] of keys[i] (zeros if absent).  One
// 32-lane half wave per key: every lane probes the same key (one broadcast
// load per probe), then lane c moves cells c, c + 32, ... so a row's reads
// and its dense output row are contiguous across the lanes.
__global__ void gather_dense_kernel(const unsigned long long *gkeys, const unsigned long long *gcounts,
                                    RowGeom g, const uint64_t *keys, uint64_t n, uint64_t *rows) {
  const uint32_t nbk = g.nbk, ostride = nbk + 1, c0 = threadIdx.x & 31u;
  for (uint64_t i = (blockIdx.x * (uint64_t)blockDim.x + threadIdx.x) >> 5; i < n;
       i += ((uint64_t)gridDim.x * blockDim.x) >> 5) {
    const uint64_t k = keys[i];
    const uint32_t s = k ? geom_find(gkeys, k * g.kmul, g) : kNotFound;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(rows) + i * ostride;
    for (uint32_t c = c0; c < ostride; c += 32) {
      unsigned long long v = 0;
      if (s != kNotFound) {
        if (g.row8) {
          const unsigned long long *row = gcounts + (uint64_t)s * (kRowBytes / 8);
          v = g.base64[(uint64_t)s * ostride + c] +
              (c < nbk ? (unsigned long long)reinterpret_cast<const uint8_t *>(row + 1)[c] : row[0]);
        } else {
          const uint32_t stride = row_stride(nbk);
          const unsigned long long *row = gcounts + (uint64_t)s * stride;
          if (c < nbk) {
            v = row[row_count_cell(c)];
          } else {
            for (uint32_t q = 0; q < stride; q += 8) v += row[q];
          }
        }
      }
      out[c] = v;
    }
  }
}

// errcnt[ws][slot] += sum over workgroups of errslab[g][ws << log2cap | slot]
// (blockIdx.y = a group of kSlabGroup workgroups; no-return u64 atomics).
__global__ void reduce_errslab_kernel(const uint32_t *errslab, uint32_t G, uint64_t per_wg,
                                      uint64_t ws, uint32_t log2cap,
                                      unsigned long long *errcnt_ws) {
  const uint64_t cap = 1ULL << log2cap;
  const uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (s >= cap) return;
  const uint32_t g0 = blockIdx.y * kSlabGroup, g1 = min(G, g0 + kSlabGroup);
  unsigned long long acc = 0;
  for (uint32_t g = g0; g < g1; ++g) acc += errslab[g * per_wg + (ws << log2cap) + s];
  if (acc) atomicAdd(errcnt_ws + s, acc);
}

__global__ void count_keys_kernel(const unsigned long long *gkeys, uint64_t cap,
                                  unsigned long long *out) {
  uint32_t c = 0;
  for (uint64_t s = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; s < cap;
       s += (uint64_t)gridDim.x * blockDim.x)
    c += gkeys[s] != 0;
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// Window read: add the exact per-slot error counts of window slot `ws` into
// its count-min cells, then clear them (so reads are idempotent).
__global__ void fold_errcnt_kernel(const unsigned long long *gkeys, unsigned long long *errcnt,
                                   uint64_t cap, unsigned long long *cms, uint32_t d, uint32_t w,
                                   uint32_t shift, const uint64_t *seeds, uint64_t kinv, uint32_t dense) {
  fold_errcnt_slots(gkeys, errcnt, cap, cms, d, w, shift, seeds, kinv, dense);
}

uint32_t grid_for(uint64_t work, uint32_t block, uint32_t cap_blocks) {
  uint64_t g = (work + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap_blocks) g = cap_blocks;
  return (uint32_t)g;
}

}  // namespace

hipError_t launch_reduce_slabs(uint32_t *slab_cnt, unsigned long long *slab_sum,
                               unsigned long long *gcounts, uint32_t G, uint64_t cap,
                               uint32_t nbk, hipStream_t s) {
  const uint32_t block = 256;
  const uint64_t srow = (nbk + 1) & ~1u, work = cap * srow / 4 + cap;
  const dim3 grid((uint32_t)((work + block - 1) / block), (G + kSlabGroup - 1) / kSlabGroup);
  hipLaunchKernelGGL(reduce_slabs_kernel, grid, dim3(block), 0, s, slab_cnt, slab_sum, gcounts, G,
                     cap, nbk);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  if (hipError_t e = hipMemsetAsync(slab_cnt, 0, (size_t)G * cap * srow * 4, s); e != hipSuccess)
    return e;
  return hipMemsetAsync(slab_sum, 0, (size_t)G * cap * 8, s);
}

hipError_t launch_compact(const unsigned long long *gkeys, unsigned long long *gcounts,
                          uint64_t cap, const RowGeom &g, unsigned long long *out_keys,
                          unsigned long long *out_rows, unsigned long long *out_n,
                          uint64_t out_cap, int reset, hipStream_t s) {
  const uint32_t block = 256;
  hipLaunchKernelGGL(compact_kernel, dim3(grid_for(cap, block, 4096)), dim3(block), 0, s, gkeys,
                     gcounts, cap, g, out_keys, out_rows, out_n, out_cap, reset);
  return hipGetLastError();
}

hipError_t launch_gather_dense(const unsigned long long *gkeys, const unsigned long long *gcounts,
                               const RowGeom &g, const uint64_t *keys, uint64_t n, uint64_t *rows,
                               hipStream_t s) {
  if (n == 0) return hipSuccess;
  const uint32_t block = 256;
  hipLaunchKernelGGL(gather_dense_kernel, dim3(grid_for(n * 32, block, 8192)), dim3(block), 0, s,  // (32 lanes a key)
                     gkeys, gcounts, g, keys, n, rows);
  return hipGetLastError();
}

hipError_t launch_fold_errcnt(const unsigned long long *gkeys, unsigned long long *errcnt,
                              uint64_t cap, unsigned long long *cms, uint32_t d, uint32_t w,
                              uint32_t shift, const uint64_t *seeds, uint64_t kinv, uint32_t dense,
                              hipStream_t s) {
  const uint32_t block = 256;
  hipLaunchKernelGGL(fold_errcnt_kernel, dim3(grid_for(cap, block, 2048)), dim3(block), 0, s, gkeys,
                     errcnt, cap, cms, d, w, shift, seeds, kinv, dense);
  return hipGetLastError();
}

hipError_t launch_reduce_errslab(uint32_t *errslab, uint32_t G, uint64_t per_wg, uint64_t ws,
                                 uint32_t log2cap, unsigned long long *errcnt_ws, hipStream_t s) {
  const uint32_t block = 256;
  const uint64_t cap = 1ULL << log2cap;
  const dim3 grid((uint32_t)((cap + block - 1) / block), (G + kSlabGroup - 1) / kSlabGroup);
  hipLaunchKernelGGL(reduce_errslab_kernel, grid, dim3(block), 0, s, errslab, G, per_wg, ws, log2cap,
                     errcnt_ws);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  // clear window ws's cells of every workgroup slab (a strided 2-D memset)
  return hipMemset2DAsync(errslab + (ws << log2cap), per_wg * 4, 0, cap * 4, G, s);
}

hipError_t launch_count_keys(const unsigned long long *gkeys, uint64_t cap,
                             unsigned long long *out, hipStream_t s) {
  const uint32_t block = 256;
  hipLaunchKernelGGL(count_keys_kernel, dim3(grid_for(cap, block, 2048)), dim3(block), 0, s,
                     gkeys, cap, out);
  return hipGetLastError();
}

}  // namespace sa
