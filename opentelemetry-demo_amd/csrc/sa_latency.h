// sa_latency.h -- the latency histogram's bin rule (include/spanagg.h, "duration
// quantiles over the window ring"), shared by the ingest kernel, the host
// helpers sa_latency_bin / sa_latency_bin_bounds and tools/latency_bins_check.cpp.
// Plain C++: no HIP header, so a host compiler takes it alone.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define SA_LAT_HD __host__ __device__
#else
#define SA_LAT_HD
#endif

namespace sa {

constexpr uint32_t kLatBins = 256;

// q = d >> 7.  q < 16: bin q (128 ns wide).  Else e = floor(log2 q) and the bin
// is ((e - 3) << 3) + (q >> (e - 3)), at most 255: eight bins an octave, the
// three bits below q's leading one.
SA_LAT_HD inline uint32_t latency_bin(uint64_t d_ns) {
  const uint64_t q = d_ns >> 7;
  if (q < 16) return (uint32_t)q;
  const uint32_t e = 63u - (uint32_t)__builtin_clzll(q);
  const uint32_t b = ((e - 3u) << 3) + (uint32_t)(q >> (e - 3u));
  return b < kLatBins - 1 ? b : kLatBins - 1;
}

// [*lo, *hi] of bin < 256, inclusive; the last bin ends at UINT64_MAX.
SA_LAT_HD inline void latency_bin_bounds(uint32_t bin, uint64_t *lo, uint64_t *hi) {
  if (bin < 16) {
    *lo = (uint64_t)bin << 7;
    *hi = *lo + 127;
    return;
  }
  const uint32_t e = (bin >> 3) + 2, m = bin & 7;
  *lo = ((uint64_t)(8 + m) << (e - 3)) << 7;
  *hi = bin == kLatBins - 1 ? UINT64_MAX : (((uint64_t)(9 + m) << (e - 3)) << 7) - 1;
}

}  // namespace sa
