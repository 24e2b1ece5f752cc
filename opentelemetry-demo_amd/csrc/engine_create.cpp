// engine_create.cpp -- C-ABI of libspanagg (include/spanagg.h): config
// validation, the path decision (sa_path.h), engine creation and destruction.
// One engine owns one gfx950 device; the product path has no CPU fallback --
// sa_create fails with SA_EDEVICE when no gfx950 device is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>

#include "sa_engine.h"
#include "sa_latency.h"
#include "spanagg_diag.h"

using sa::Path;

namespace {

constexpr double kDefaultBounds[16] = {2,   4,   6,    8,    10,   50,   100,   200,
                                       400, 800, 1000, 1400, 2000, 5000, 10000, 15000};
constexpr uint64_t kCmsSeed[8] = {0x9E3779B97F4A7C15ULL, 0xBF58476D1CE4E5B9ULL,
                                  0x94D049BB133111EBULL, 0xD6E8FEB86659FD93ULL,
                                  0xA0761D6478BD642FULL, 0xE7037ED1A0B428DBULL,
                                  0x8EBC6AF09C88C6E3ULL, 0x589965CC75374CC3ULL};
constexpr uint32_t kDefaultSlabSets = 2;  // SPANAGG_SLAB_SETS overrides (laboratory build)

// The engine's ordering events only order its own launches, copies and
// reads on this device (cross-stream waits, slab-set and record-set reuse),
// so they release at device scope: a default event ends with a system-scope
// fence (L2 write-back and invalidate) that the next launch on the stream
// waits behind and starts cold after.  (Laboratory build: SPANAGG_EV_SYS=1
// restores the default for A/B runs.)
unsigned ev_flags() {
  return lab().ev_sys ? hipEventDisableTiming : (hipEventDisableTiming | hipEventReleaseToDevice);
}

bool is_pow2(uint64_t x) { return x && !(x & (x - 1)); }

// Checks the config and builds its histogram (thresholds and bin table) into h.
int validate_config(const sa_config *c, sa::Hist &h, std::string &why) {
  if (!c) return why = "null config", SA_EINVAL;
  if (c->n_bounds > SA_MAX_BOUNDS) return why = "too many histogram bounds", SA_EINVAL;
  if (c->n_bounds && !c->bounds) return why = "bounds pointer is null", SA_EINVAL;
  if (c->unit > SA_UNIT_S) return why = "unit must be ms or s", SA_EINVAL;
  if (c->hll_p < 4 || c->hll_p > 18) return why = "hll_p must be in 4..18", SA_EINVAL;
  if (c->cms_d < 1 || c->cms_d > 8) return why = "cms_d must be in 1..8", SA_EINVAL;
  if (c->cms_w < 2 || !is_pow2(c->cms_w)) return why = "cms_w must be a power of two >= 2", SA_EINVAL;
  if (c->window_ns == 0) return why = "window_ns must be > 0", SA_EINVAL;
  if (c->window_ns >> 56) return why = "window_ns must stay below 2^56 ns (~2.3 years)", SA_EINVAL;
  if (!is_pow2(c->n_windows) || c->n_windows > 4096)
    return why = "n_windows must be a power of two <= 4096", SA_EINVAL;
  if (c->n_services < 1 || c->n_services > 65536)
    return why = "n_services must be in 1..65536", SA_EINVAL;
  if (c->key_capacity < 1 || c->key_capacity > (1ULL << 30))
    return why = "key_capacity must be in 1..2^30", SA_EINVAL;
  if (c->window_ns >= (1ULL << 63) / c->n_windows)
    return why = "n_windows * window_ns must stay below 2^63 ns", SA_EINVAL;
  if (((uint64_t)c->n_windows * c->n_services << c->hll_p) >= (1ULL << 32))
    return why = "n_windows * n_services * 2^hll_p must stay below 2^32 registers", SA_EINVAL;
  if (c->exp_max_size == 1 || c->exp_max_size > sa::kExpoMaxSize)
    return why = "exp_max_size must be 0 (explicit buckets) or 2..4096", SA_EINVAL;
  if (c->options & ~SA_OPT_ALL) return why = "unknown bits in options", SA_EINVAL;
  if ((c->options & SA_OPT_WINDOW_LATENCY) && (uint64_t)c->n_windows * c->n_services > (1ULL << 18))
    return why = "SA_OPT_WINDOW_LATENCY: n_windows * n_services must stay within 2^18 (a 512 MiB ring)", SA_EINVAL;
#ifndef SPANAGG_AB
  if (c->flags) return why = "SA_DIAG_* flags need the laboratory build (libspanagg_ab.so)", SA_EINVAL;
#endif
  const bool sorted = sa::build_hist(c->bounds, c->n_bounds, c->unit, h);
  if (c->options & SA_OPT_DENSE_IDS) {
    if (c->exp_max_size != 0) return why = "SA_OPT_DENSE_IDS: explicit buckets only (exp_max_size must be 0)", SA_EINVAL;
    if (c->n_bounds + 1 > sa::kPartMaxBk) return why = "SA_OPT_DENSE_IDS: at most 17 buckets (16 bounds)", SA_EINVAL;
    if (c->n_windows > 1024) return why = "SA_OPT_DENSE_IDS: n_windows must be <= 1024", SA_EINVAL;
    if (c->options & (SA_OPT_PARTITIONED | SA_OPT_ATOMIC_TABLE | SA_OPT_EXPO_HBM | SA_OPT_EXPO_CACHED))
      return why = "SA_OPT_DENSE_IDS cannot be combined with another table path option", SA_EINVAL;
    if (sa::dense_table_slots(c->key_capacity) > (1ULL << 22))
      return why = "SA_OPT_DENSE_IDS: key_capacity needs a table above 2^22 slots", SA_EINVAL;
    if (!sorted || !h.has_bins) return why = "SA_OPT_DENSE_IDS: the bounds do not fit the bucket bin table", SA_EINVAL;
  }
  if (!sorted) return why = "histogram bounds must be sorted ascending and not NaN", SA_EINVAL;
  return SA_OK;
}

}  // namespace

extern "C" {

int sa_abi_version(void) { return SA_ABI_VERSION; }

void sa_config_default(sa_config *c) {
  if (!c) return;
  std::memset(c, 0, sizeof *c);
  c->bounds = kDefaultBounds;
  c->n_bounds = 16;
  c->unit = SA_UNIT_MS;
  c->hll_p = 14;
  c->cms_d = 4;
  c->cms_w = 2048;
  c->window_ns = 10ULL * 1000000000ULL;
  c->n_windows = 8;
  c->n_services = 64;
  c->key_capacity = 1000;  // the connector's dimensions_cache_size default
  c->device = 0;
}

int sa_bucket_thresholds(const double *bounds, uint32_t n, uint32_t unit, uint64_t *thr,
                         uint32_t *n_neg) {
  return sa::bucket_thresholds(bounds, n, unit, thr, n_neg);
}

double sa_hll_estimate(const uint8_t *regs, uint32_t p) {
  if (!regs || p < 4 || p > 18) return -1.0;
  const uint32_t m = 1u << p;
  double sum = 0.0;
  uint32_t zeros = 0;
  for (uint32_t j = 0; j < m; ++j) {
    sum += std::ldexp(1.0, -(int)regs[j]);
    zeros += regs[j] == 0;
  }
  const double alpha = m == 16 ? 0.673 : m == 32 ? 0.697 : m == 64 ? 0.709
                                                                  : 0.7213 / (1.0 + 1.079 / m);
  double est = alpha * (double)m * (double)m / sum;
  if (est <= 2.5 * m && zeros) est = (double)m * std::log((double)m / (double)zeros);
  return est;
}

double sa_hll_estimate_hist(const uint32_t *hist, uint32_t p) {
  if (!hist || p < 4 || p > 18) return -1.0;
  const uint32_t m = 1u << p;
  // sum hist[v] * 2^-v, exactly: 2^63 times it is an integer below 2^(32 + 63)
  unsigned __int128 acc = 0;
  for (uint32_t v = 0; v < SA_HLL_HIST_BINS; ++v) acc += (unsigned __int128)hist[v] << (63 - v);
  const double sum = std::ldexp((double)acc, -63);
  const uint32_t zeros = hist[0];
  const double alpha = m == 16 ? 0.673 : m == 32 ? 0.697 : m == 64 ? 0.709
                                                                  : 0.7213 / (1.0 + 1.079 / m);
  double est = alpha * (double)m * (double)m / sum;
  if (est <= 2.5 * m && zeros) est = (double)m * std::log((double)m / (double)zeros);
  return est;
}

uint32_t sa_latency_bin(uint64_t d_ns) { return sa::latency_bin(d_ns); }

int sa_latency_bin_bounds(uint32_t bin, uint64_t *lo, uint64_t *hi) {
  if (bin >= SA_LAT_BINS || !lo || !hi) return SA_EINVAL;
  sa::latency_bin_bounds(bin, lo, hi);
  return SA_OK;
}

int sa_create(const sa_config *cfg, sa_engine **out) {
  if (!out) return SA_EINVAL;
  *out = nullptr;
  auto *e = new sa_engine();
  std::string why;
  if (int rc = validate_config(cfg, e->hist, why)) {
    std::fprintf(stderr, "sa_create: %s\n", why.c_str());
    delete e;
    return rc;
  }
  const LabKnobs knobs = lab_for_create();  // (laboratory build: this engine's SPANAGG_SLAB_SETS, SPANAGG_KMUL, ...)
  e->cfg = *cfg;
  e->cfg.bounds = e->hist.bounds.data();
  const sa::Hist &h = e->hist;

  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 ||
      cfg->device >= ndev) {
    std::fprintf(stderr, "sa_create: no HIP device %d (found %d)\n", cfg->device, ndev);
    delete e;
    return SA_EDEVICE;
  }
  e->dev = cfg->device;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, e->dev) != hipSuccess ||
      std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    std::fprintf(stderr, "sa_create: device %d is not gfx950 (%s)\n", e->dev, prop.gcnArchName);
    delete e;
    return SA_EDEVICE;
  }
  e->cus = (uint32_t)prop.multiProcessorCount;

  auto bail = [&](int rc) {
    std::fprintf(stderr, "sa_create: %s\n", e->err.c_str());
    sa_destroy(e);
    return rc;
  };
  auto lds_attr = [&](hipError_t st) {
    return st == hipSuccess ? SA_OK : fail(e, SA_EDEVICE, std::string("LDS attribute: ") + hipGetErrorString(st));
  };
  auto event = [&](hipEvent_t &ev) {
    return (ev = e->res.new_event(ev_flags())) ? SA_OK : fail(e, SA_EDEVICE, "event creation failed");
  };
  if (int rc = set_dev(e)) return bail(rc);
  // A blocking stream: it orders against the legacy null stream, so callers
  // that produce batches on the null stream (stream == NULL) stay race-free.
  if (!(e->stream = e->res.new_stream(hipStreamDefault)) || event(e->ev_a) || event(e->ev_b) || event(e->order.ev_ctl))
    return bail(fail(e, SA_EDEVICE, "stream/event creation failed"));
  int rc = SA_OK;
  for (hipEvent_t &ev : e->order.ev_set)
    if ((rc = event(ev))) return bail(rc);

  // buckets of 4 slots with two choices stay well-behaved up to ~90% load:
  // size for 80% at the declared capacity (the LDS mirror path needs cap <= 2048)
  e->cap = sa::config_table_slots(*cfg);
  e->log2cap = sa::log2u(e->cap);
  const sa::PathChoice choice = sa::decide_path(*cfg, h, e->cap);
  e->path = choice.path;
  e->lds_bytes = choice.lds_bytes;
  const bool small = e->path == Path::Small, expo_small = e->path == Path::ExpoSmall;
  if (small) {
    // the kernel for the geometry (sa_path.h small_kernel).  Laboratory build:
    // an engine with SA_DIAG_* flags runs the ablation instance, which has
    // Generic1024's geometry, and reports SA_KERNEL_LAB
    sa::SmallKernel k = sa::small_kernel(h.has_bins, e->lds_bytes, e->log2cap, h.nbk, cfg->hll_p);
    if (e->diag() && k == sa::SmallKernel::Linear)
      return bail(fail(e, SA_EINVAL, "SA_DIAG_* flags: the linear-threshold kernel has no ablation instance"));
    if (e->diag()) k = sa::SmallKernel::Generic1024;
    e->small_kernel = k;
    e->kernel_kind = e->diag()                          ? SA_KERNEL_LAB
                     : k == sa::SmallKernel::Default    ? SA_KERNEL_SMALL_DEFAULT
                     : k == sa::SmallKernel::Generic512 ? SA_KERNEL_SMALL_512
                     : k == sa::SmallKernel::Generic1024 ? SA_KERNEL_SMALL_1024
                                                         : SA_KERNEL_SMALL_LINEAR;
    e->spl = sa::small_spans_per_lane(k);
    e->block = sa::small_block(k);
    if ((rc = lds_attr(sa::prepare_ingest_small(e->lds_bytes)))) return bail(rc);
    // one resident round of workgroups (registers and LDS decide how many
    // share a CU; a second round would repeat every workgroup's prologue)
    uint32_t per_cu = sa::ingest_small_blocks_per_cu(k, e->diag(), e->lds_bytes);
    if (per_cu == 0)
      per_cu = std::max<uint32_t>(1, std::min<uint32_t>(2048 / e->block, (uint32_t)((160 * 1024) / e->lds_bytes)));
    e->G = e->cus * per_cu;
  } else if (expo_small) {
    e->kernel_kind = sa::expo_kernel(e->log2cap, cfg->hll_p) == sa::ExpoKernel::Specialised ? SA_KERNEL_EXPO_SPECIALISED
                                                                                            : SA_KERNEL_EXPO_GENERIC;
    e->block = 1024;
    e->spl = 2;
    if ((rc = lds_attr(sa::prepare_ingest_expo_small(e->lds_bytes)))) return bail(rc);
    // one resident round of workgroups (registers and LDS), as the small tables
    uint32_t per_cu = sa::ingest_expo_blocks_per_cu(e->log2cap, cfg->hll_p, e->lds_bytes);
    if (per_cu == 0) per_cu = std::max<uint32_t>(1, (uint32_t)((160 * 1024) / e->lds_bytes));
    e->G = e->cus * per_cu;
    if ((rc = lds_attr(sa::prepare_expo_count(sa::expo_count_lds_bytes(e->cap, cfg->exp_max_size))))) return bail(rc);
    // slab counting: its workgroups (one per ingest workgroup) share a CU as the
    // ingest ones do; SA_OPT_EXPO_CACHED keeps the cached-probe kernel
    const size_t budget = (size_t)160 * 1024 * e->cus / e->G - 1024;
    e->expo.xc_ne = (cfg->options & SA_OPT_EXPO_CACHED) ? 0u : sa::expo_slab_entries(e->cap, cfg->exp_max_size, budget);
    if (e->expo.xc_ne &&
        (rc = lds_attr(sa::prepare_expo_slab(sa::expo_slab_lds_bytes(e->cap, cfg->exp_max_size, e->expo.xc_ne)))))
      return bail(rc);
  } else {
    // (the binned and dense scatters have one instance: the value names the bounds they run with)
    e->kernel_kind = sa::bounds16(h.nneg, h.npos) ? SA_KERNEL_BOUNDS16 : SA_KERNEL_BOUNDS_GENERIC;
    e->block = sa::kHbmBlock;
    e->spl = sa::kHbmSpansPerLane;
    e->G = e->cus * 8;
    // (the binned path keeps the partitioned kernels' attribute too)
    if (e->path == Path::Partitioned || e->path == Path::Binned)
      if ((rc = lds_attr(sa::prepare_ingest_part()))) return bail(rc);
  }
  const bool binned = sa::binned_like(e->path);

  const uint64_t S = cfg->n_services, W = cfg->n_windows;
  e->hll_slot_bytes = (size_t)S << cfg->hll_p;
  e->cms_slot_elems = (size_t)cfg->cms_d * cfg->cms_w;
  const size_t count_words = binned ? (size_t)e->cap * sa::kRowBytes / 8 : (size_t)e->cap * sa::row_stride(h.nbk);
  if ((rc = dalloc(e, e->gkeys, e->cap, true)) || (rc = dalloc(e, e->gcounts, count_words, true)) ||
      (rc = dalloc(e, e->hll, e->hll_slot_bytes * W, true)) ||
      (rc = dalloc(e, e->cms, e->cms_slot_elems * W, true)) ||
      (rc = dalloc(e, e->errcnt, (size_t)W * e->cap, true)) || (rc = dalloc(e, e->d_seeds, 8, true)) ||
      (rc = dalloc(e, e->stats, 8, true)) || (rc = dalloc(e, e->scratch, 8, true)) ||
      (rc = dalloc(e, e->hll_filt, sa::kFiltSlots, true)))
    return bail(rc);
  {
    // bound sub-blocks: as small as kLbMinShift allows within kLbMaxSub of them
    // (SA_OPT_NO_HLL_FILTER turns the filter off)
    const sa::LbGeom lb = sa::hll_filter_geometry(*cfg);
    if (lb.n) {
      e->lb_shift = lb.shift;
      e->lb_n = lb.n;
      if ((rc = dalloc(e, e->hll_lb, ((size_t)e->lb_n + 15) & ~(size_t)15, true))) return bail(rc);
    }
  }
  if (small || expo_small) e->order.nsets = knobs.slab_sets ? knobs.slab_sets : kDefaultSlabSets;
  if (sa::expo_like(e->path)) {
    sa_engine::Expo &x = e->expo;
    const uint32_t M = cfg->exp_max_size;
    if ((rc = dalloc(e, x.hdr, e->cap, true)) || (rc = dalloc(e, x.buckets, (size_t)2 * e->cap * M, true)))
      return bail(rc);
    if (expo_small && (rc = dalloc(e, x.xscale, e->cap, true))) return bail(rc);
    if (sa::launch_expo_init(x.hdr, x.xscale, e->cap, nullptr) != hipSuccess)
      return bail(fail(e, SA_EDEVICE, "expo state init failed"));
    if (expo_small) {
      const size_t gs = (size_t)e->order.nsets * e->G;
      if ((rc = dalloc(e, x.xslab, gs * e->cap, true)) || (rc = event(x.ev_expo))) return bail(rc);
      // (laboratory build, SPANAGG_XSTREAM=1: the histogram kernels on an
      // engine stream -- slower by A/B)
      x.xidx = knobs.xidx;
      if (knobs.xstream) {
        if (!(x.xstream = e->res.new_stream(hipStreamNonBlocking)))
          return bail(fail(e, SA_EDEVICE, "histogram stream creation failed"));
        for (hipEvent_t &ev : x.ev_ing)
          if ((rc = event(ev))) return bail(rc);
      }
      if (x.xc_ne &&
          ((rc = dalloc(e, x.xc_lcount, e->cap * 3, true)) ||  // lcount [cap], then xmeta [cap]
           (rc = dalloc(e, x.xc_slot_of_entry, (size_t)x.xc_ne * 2, true)) ||
           (rc = dalloc(e, x.xc_ent, (size_t)e->cap * 2, true)) ||
           (rc = dalloc(e, x.xcslab, (size_t)e->G * sa::xc_slab_stride(x.xc_ne, M), true)) ||
           (rc = dalloc(e, x.xt_rec, (size_t)e->G * sa::xt_bins(e->cap, M) * sa::kXtRun, true)) ||
           (rc = dalloc(e, x.xt_off, (size_t)e->G * (sa::xt_bins(e->cap, M) + 1), true))))
        return bail(rc);
      // no selection yet: no entries (the first launch counts every span through the tail)
      if (x.xc_ne && (hipMemset(x.xc_slot_of_entry, 0xFF, (size_t)x.xc_ne * 8) != hipSuccess ||
                      hipMemset(x.xc_ent, 0xFF, (size_t)e->cap * 8) != hipSuccess))
        return bail(fail(e, SA_EDEVICE, "hipMemset failed"));
      // (window, slot) keys of the LDS ERROR table are 16-bit
      if (sa::error_table(cfg->n_windows, e->cap) &&
          (rc = dalloc(e, e->small.errslab, gs * cfg->n_windows * e->cap, true)))
        return bail(rc);
    }
  }
  if ((cfg->options & SA_OPT_STAMPS) && (rc = dalloc(e, e->dbg, (size_t)e->G * sa::kDbgPerWg, true)))
    return bail(rc);
  if (cfg->options & SA_OPT_WINDOW_LATENCY) {
    sa_engine::Latency &L = e->lat;
    if ((rc = dalloc(e, L.ring, (size_t)W * S * SA_LAT_BINS, true, "latency ring hipMalloc failed"))) return bail(rc);
    const sa::LatGeom lg = sa::lat_geometry(cfg->n_services, cfg->n_windows);
    L.k_slots = lg.k_slots;
    L.grid_max = e->cus * lg.per_cu;
    if (L.k_slots && (rc = lds_attr(sa::prepare_lat_ingest((size_t)L.k_slots * cfg->n_services * 1024)))) return bail(rc);
  }
  if (h.has_bins) {
    if ((rc = dalloc(e, e->d_bins, sa::kBins, true))) return bail(rc);
    if (hipMemcpy(e->d_bins, h.bins, sizeof h.bins, hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(e, SA_EDEVICE, "bin table upload failed"));
  }
  if (binned) {
    sa_engine::Binned &b = e->binned;
    const bool dense = e->dense();
    // one scatter workgroup per CU (~160 KiB LDS); 512-thread aggregate
    // workgroups sized for the bin's sub-table
    b.log2sb = e->log2cap - sa::kPartBinBits;
    b.grid = e->cus;
    b.agg_lds = dense ? sa::dn_agg_lds_bytes(b.log2sb, b.grid) : sa::bt_agg2_lds_bytes(b.log2sb, b.grid);
    // the dense aggregate's u16 LDS counters: a bin's records of two record
    // sets at the largest launch must stay below 2^16 (spanagg_dense.hip)
    if (dense && 2ull * b.grid * bt_region_for(e, sa::kBtMaxWgSpans) > 65535)
      return bail(fail(e, SA_EINVAL, "SA_OPT_DENSE_IDS: too many compute units for the aggregate's u16 counters"));
    if ((rc = dalloc(e, b.base64, (size_t)e->cap * (h.nbk + 1), true))) return bail(rc);  // (the spill array)
    if (dense) b.bound.assign((e->cap + 63) / 64, 0);
    if ((rc = lds_attr(dense ? sa::prepare_ingest_dn(b.agg_lds) : sa::prepare_ingest_bt(b.agg_lds)))) return bail(rc);
    // the aggregate stream of the launch pipeline (ordered by events only)
    if (!(b.agg_stream = e->res.new_stream(hipStreamNonBlocking)))
      return bail(fail(e, SA_EDEVICE, "aggregate stream creation failed"));
    for (int k = 0; k < sa_engine::Binned::kSets; ++k)
      if ((rc = event(b.ev_scat[k])) || (rc = event(b.ev_agg[k]))) return bail(rc);
    // a random odd multiplier per engine: series ids -> stored ids (bins and
    // home slots), so bin occupancy does not depend on ids a sender chooses
    std::random_device rd;
    uint64_t r = ((uint64_t)rd() << 32) ^ rd();
    if ((cfg->options & SA_OPT_IDENTITY_IDS) || dense) r = 1;  // stored id = series id (tests of a full bin)
    if (knobs.kmul_set && !dense) r = knobs.kmul;  // fixed, for A/B runs
    b.kmul = r | 1ULL;
    uint64_t x = b.kmul;  // Newton: x = x (2 - a x) doubles the correct low bits
    for (int i = 0; i < 6; ++i) x *= 2 - b.kmul * x;
    b.kinv = x;
  }
  if (hipMemcpy(e->d_seeds, kCmsSeed, sizeof kCmsSeed, hipMemcpyHostToDevice) != hipSuccess)
    return bail(fail(e, SA_EDEVICE, "seed upload failed"));
  if (small) {
    sa_engine::Small &s = e->small;
    const size_t srow = (h.nbk + 1) & ~1u;  // slab row = 2 * ceil(nbk/2) u32 cells
    const size_t gs = (size_t)e->G * e->order.nsets;  // slabs of all sets, set-major
    if ((rc = dalloc(e, s.slab_cnt, gs * e->cap * srow, true)) || (rc = dalloc(e, s.slab_sum, gs * e->cap, true)))
      return bail(rc);
    // (window, slot) keys of the v2 kernels' LDS ERROR table are 16-bit (the
    // linear-threshold kernel counts ERROR spans per span: its slabs stay zero)
    if (sa::error_table(cfg->n_windows, e->cap) &&
        (rc = dalloc(e, s.errslab, gs * cfg->n_windows * e->cap, true)))
      return bail(rc);
  }
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(e, SA_EDEVICE, "device sync failed"));
  *out = e;
  return SA_OK;
}

// Waits for the engine's work (every set joined onto the engine stream), then
// releases everything the engine made, newest first.
void sa_destroy(sa_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->dev);
  if (e->stream) {
    join_sets(e);
    (void)hipStreamSynchronize(e->stream);
  }
  for (auto &g : e->small.gi) {
    if (g.x) (void)hipGraphExecDestroy(g.x);
    if (g.g) (void)hipGraphDestroy(g.g);
  }
  e->res.release_all();
  delete e;
}

const char *sa_last_error(const sa_engine *e) { return e ? e->err.c_str() : "null engine"; }

int sa_debug_geometry(sa_engine *e, sa_debug_geometry_info *out) {
  if (!e || !out) return SA_EINVAL;
  std::memset(out, 0, sizeof *out);
  out->path = (uint32_t)e->path;
  out->kernel = (uint32_t)e->kernel_kind;
  // (the binned, dense and partitioned scatters have blocks and grids of their own)
  const bool part = e->path == Path::Partitioned;
  out->block = sa::binned_like(e->path) ? sa::kBtBlock : part ? sa::kPartBlock : e->block;
  out->grid_max = sa::binned_like(e->path) ? e->binned.grid : part ? sa::kPartMaxGrid : e->G;
  out->log2cap = e->log2cap;
  out->lb_shift = e->lb_shift;
  out->lb_n = e->lb_n;
  out->error_table = e->small.errslab != nullptr;
  out->lds_bytes = sa::lds_table(e->path) ? e->lds_bytes : 0;
  if (e->path == Path::ExpoHbm) {
    out->expo_count = SA_EXPO_COUNT_HBM;
  } else if (e->path == Path::ExpoSmall && e->expo.xc_ne) {
    const uint32_t M = e->cfg.exp_max_size;
    out->expo_count = SA_EXPO_COUNT_SLAB;
    out->expo_entries = e->expo.xc_ne;
    out->expo_bin_slots = sa::xt_bin_slots(M);
    out->expo_bins = sa::xt_bins(e->cap, M);
  } else if (e->path == Path::ExpoSmall) {
    out->expo_count = SA_EXPO_COUNT_CACHED;
    out->expo_entries = sa::expo_cached_entries(e->cfg.exp_max_size);
  }
  return SA_OK;
}

}  // extern "C"
