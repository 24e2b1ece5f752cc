// sa_shard.h -- what an engine group decides without a device (include/spanagg.h,
// sa_group_*): the member a span goes to, and the fold of the members'
// exponential histograms into one.  Shared by csrc/spanagg_group.cpp (the host
// split, the partition kernels, sa_group_flush_exp) and the stand-alone
// programs of tests/test_group_host.py.
// Plain C++: no HIP header, so a host compiler takes it alone.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "spanagg.h"

#if defined(__HIPCC__)
#define SA_SHARD_HD __host__ __device__
#else
#define SA_SHARD_HD
#endif

namespace sa {

constexpr uint32_t kMaxMembers = 64;

// ---- trace-id sharding (engine = trace_w1 % n) ------------------------------
// trace_w1 % n from 32-bit remainders: w1 = hi * 2^32 + lo, so
// w1 % n = ((hi % n) * (2^32 % n) + lo % n) % n (< n^2 <= 4096 before the
// last remainder); no 64-bit division per span.  r32 = 2^32 % n.
SA_SHARD_HD inline uint32_t shard_of(uint64_t w1, uint32_t n, uint32_t r32) {
  return (((uint32_t)(w1 >> 32) % n) * r32 + (uint32_t)w1 % n) % n;
}

// One series' exponential histogram while members' deltas are folded in.
struct ExpoAcc {
  uint64_t count = 0, zero = 0, sum_ns = 0;
  double min = 0, max = 0;
  int32_t scale = 20, offset = 0;  // go-expohisto's initial scale
  std::vector<uint64_t> c;         // positive buckets offset .. offset + size - 1
};

inline int64_t shr_floor(int64_t v, int k) { return v >= 0 ? v >> k : -((-v - 1) >> k) - 1; }

// Folds one member's histogram into a: go-expohisto's state depends only on
// the values, and index(v) at scale s is index(v) at scale s + k shifted
// right by k, so both go to the smaller scale, the index ranges unite and
// the least further downscale that fits max_size applies (changeScale) --
// exactly the histogram one engine fed both members' spans would hold.
inline void expo_fold(ExpoAcc &a, const sa_exp_result &r, uint64_t j, uint32_t max_size) {
  if (r.count[j] == 0) return;
  if (a.count == 0) {
    a.min = r.min[j];
    a.max = r.max[j];
  } else {
    a.min = std::min(a.min, r.min[j]);
    a.max = std::max(a.max, r.max[j]);
  }
  a.count += r.count[j];
  a.zero += r.zero_count[j];
  a.sum_ns += r.sum_ns[j];
  const uint32_t nb = r.n_buckets[j];
  const uint64_t *cnt = r.bucket_counts + j * r.max_size;
  if (nb == 0) return;
  if (a.c.empty()) {
    a.scale = r.scale[j];
    a.offset = r.offset[j];
    a.c.assign(cnt, cnt + nb);
    return;
  }
  int s = std::min(a.scale, r.scale[j]);
  const int ka = a.scale - s, kd = r.scale[j] - s;
  int64_t lo = std::min(shr_floor(a.offset, ka), shr_floor(r.offset[j], kd));
  int64_t hi = std::max(shr_floor((int64_t)a.offset + (int64_t)a.c.size() - 1, ka),
                        shr_floor((int64_t)r.offset[j] + nb - 1, kd));
  int c = 0;
  while (hi - lo >= (int64_t)max_size) lo = shr_floor(lo, 1), hi = shr_floor(hi, 1), ++c;
  std::vector<uint64_t> out((size_t)(hi - lo + 1), 0);
  for (size_t i = 0; i < a.c.size(); ++i) out[(size_t)(shr_floor((int64_t)a.offset + (int64_t)i, ka + c) - lo)] += a.c[i];
  for (uint32_t i = 0; i < nb; ++i) out[(size_t)(shr_floor((int64_t)r.offset[j] + i, kd + c) - lo)] += cnt[i];
  a.scale = s - c;
  a.offset = (int32_t)lo;
  a.c.swap(out);
}

}  // namespace sa
