// engine_read.cpp -- the read side of the engine: flush and compaction,
// window sketches and range queries over them, stats, key reclamation, the merge hooks (export, gather),
// sa_bind_ids, the probes and the engine group's asynchronous hooks (sa_grp).
// Every call here joins the launches in flight onto the engine stream first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <new>
#include <numeric>
#include <string>
#include <tuple>
#include <vector>

#include "sa_engine.h"
#include "sa_group_hooks.h"
#include "sa_results.h"

namespace {

size_t counts_bytes(const sa_engine *e) {
  return sa::binned_like(e->path) ? (size_t)e->cap * sa::kRowBytes : (size_t)e->cap * sa::row_stride(e->hist.nbk) * 8;
}

sa::RowGeom geom(const sa_engine *e) {
  const bool binned = sa::binned_like(e->path);
  sa::RowGeom g{};
  g.nbk = e->hist.nbk;
  g.row8 = binned ? 1u : 0u;
  g.binned = binned ? 1u : 0u;
  g.log2cap = e->log2cap;
  g.log2sb = e->binned.log2sb;
  g.max_probe = sa::max_probe_of(e->log2cap);
  g.kmul = e->binned.kmul;
  g.kinv = e->binned.kinv;
  g.base64 = e->binned.base64;
  g.dense = e->dense() ? 1u : 0u;
  g.dropped = e->stats + sa::kStatDropped;
  return g;
}

// Every read starts here: the engine's device, and every launch in flight
// joined onto the engine stream (a pending aggregate that failed is returned).
int begin_read(sa_engine *e) {
  if (int rc = set_dev(e)) return rc;
  return join_checked(e);
}

double unit_div(const sa_engine *e) { return e->cfg.unit == SA_UNIT_S ? 1e9 : 1e6; }

// A caller's stream `s` takes over from the engine stream (ev_a), and hands
// back: later engine work orders after what the caller's stream did (ev_b).
int hop_to(sa_engine *e, hipStream_t s) {
  if (s == e->stream) return SA_OK;
  SA_HIP(e, hipEventRecord(e->ev_a, e->stream));
  SA_HIP(e, hipStreamWaitEvent(s, e->ev_a, 0));
  return SA_OK;
}
int hop_back(sa_engine *e, hipStream_t s) {
  if (s == e->stream) return SA_OK;
  SA_HIP(e, hipEventRecord(e->ev_b, s));
  SA_HIP(e, hipStreamWaitEvent(e->stream, e->ev_b, 0));
  return SA_OK;
}

int read_stats(sa_engine *e, uint64_t out[sa::kNumStats]) {
  SA_HIP(e, hipMemcpyAsync(out, e->stats, sa::kNumStats * 8, hipMemcpyDeviceToHost, e->stream));
  SA_HIP(e, hipStreamSynchronize(e->stream));
  return SA_OK;
}

// Derive the count-min cells of window slot ws from its exact per-slot error
// counts (see sketch_post in sa_device.h).
int fold_errslab(sa_engine *e, uint64_t ws, hipStream_t s) {
  if (!e->small.errslab) return SA_OK;
  SA_HIP(e, sa::launch_reduce_errslab(e->small.errslab, e->G * e->order.nsets, (uint64_t)e->cfg.n_windows * e->cap, ws,
                                      e->log2cap, e->errcnt + ws * e->cap, s));
  return SA_OK;
}

int fold_window(sa_engine *e, uint64_t ws, hipStream_t s) {
  if (int rc = fold_errslab(e, ws, s)) return rc;
  SA_HIP(e, sa::launch_fold_errcnt(e->gkeys, e->errcnt + ws * e->cap, e->cap,
                                   e->cms + ws * e->cms_slot_elems, e->cfg.cms_d, e->cfg.cms_w,
                                   64 - sa::log2u(e->cfg.cms_w), e->d_seeds, e->binned.kinv, e->dense() ? 1u : 0u, s));
  return SA_OK;
}

int fold_windows(sa_engine *e) {
  for (uint32_t ws = 0; ws < e->cfg.n_windows; ++ws)
    if (int rc = fold_window(e, ws, e->stream)) return rc;
  return SA_OK;
}

// Empties the key table.  Keys are a cache of the series seen: after a flush
// every row is zero, so a forgotten key costs nothing and is re-inserted by its
// next span (the delta histograms do not depend on the slot).  Window error
// counts are kept per slot, so every resident window's are folded into its
// count-min first.
int reclaim_now(sa_engine *e) {
  if (int rc = fold_windows(e)) return rc;
  SA_HIP(e, hipMemsetAsync(e->gkeys, 0, e->cap * 8, e->stream));
  ++e->reclaims;
  return SA_OK;
}

// *nk = the resident keys (counted into scratch[slot]; the caller waits)
int count_keys(sa_engine *e, uint64_t *nk, int slot = 0) {
  SA_HIP(e, hipMemsetAsync(e->scratch + slot, 0, 8, e->stream));
  SA_HIP(e, sa::launch_count_keys(e->gkeys, e->cap, e->scratch + slot, e->stream));
  SA_HIP(e, hipMemcpyAsync(nk, e->scratch + slot, 8, hipMemcpyDeviceToHost, e->stream));
  return SA_OK;
}

// Flush-time policy: reclaim once more than half the table is resident, so a
// collector whose series churn (new pods, restarts) keeps room for the next
// interval's series instead of dropping their spans.  Binned tables reclaim
// past 35 %: their bins are as small as 256 slots, and a fully churned next
// interval doubles the load, which must stay near 70 % for no bin to fill
// (at 76 % of a 2^19-slot table, 2,048 bins of 256, P(some bin full) = 2.8 %).
int reclaim_if_full(sa_engine *e) {
  if (e->dense()) return SA_OK;  // nothing is ever full: the host owns the index space
  uint64_t nk = 0;
  if (int rc = count_keys(e, &nk)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));
  return sa_grp::over_reclaim_threshold(e, nk) ? reclaim_now(e) : SA_OK;
}

// The end of both flushes: the reclamation policy, then SA_EFULL when spans
// were dropped since the previous flush.
int finish_flush(sa_engine *e) {
  e->unflushed = false;
  if (int rc = reclaim_if_full(e)) return rc;
  uint64_t st[sa::kNumStats];
  if (int rc = read_stats(e, st)) return rc;
  if (st[sa::kStatDropped] == e->dropped_seen) return SA_OK;
  e->dropped_seen = st[sa::kStatDropped];
  if (e->dense()) {
    // spans on unbound indices: their ERROR counts go too (the fold clears
    // the cells of slots without a key), before a later bind gives the
    // index a series
    if (int rc = fold_windows(e)) return rc;
    return fail(e, SA_EFULL, "spans on an unbound or out-of-range index were dropped since the previous flush");
  }
  return fail(e, SA_EFULL, "key table full: spans were dropped since the previous flush");
}

// the rows' order by key
std::vector<uint64_t> key_order(const std::vector<uint64_t> &k) {
  std::vector<uint64_t> ord(k.size());
  std::iota(ord.begin(), ord.end(), 0);
  std::sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return k[a] < k[b]; });
  return ord;
}

// sa_export_keys' device part on `s` (after the engine's work): the resident
// keys with a non-zero delta into d_keys, their count into scratch[0]
int export_keys_on(sa_engine *e, uint64_t *d_keys, uint64_t cap, hipStream_t s) {
  if (int rc = reduce_slabs(e, s)) return rc;
  SA_HIP(e, hipMemsetAsync(e->scratch, 0, 8, s));
  SA_HIP(e, sa::launch_compact(e->gkeys, e->gcounts, e->cap, geom(e), reinterpret_cast<unsigned long long *>(d_keys),
                               nullptr, e->scratch, cap, 0, s));
  return SA_OK;
}

bool resident(const sa_engine *e, uint64_t w) {
  return w >= e->win_base && w - e->win_base < e->cfg.n_windows;
}

// ---- range queries (sa_window_range; kernels in spanagg_range.hip) ----
constexpr uint32_t kRangeFlags = SA_RANGE_REGISTERS | SA_RANGE_CELLS;

int range_args(sa_engine *e, uint64_t first, uint64_t last, const uint64_t *keys, uint64_t n_keys, uint32_t flags) {
  if (n_keys && !keys) return fail(e, SA_EINVAL, "window range: n_keys != 0 with null keys");
  if (flags & ~kRangeFlags) return fail(e, SA_EINVAL, "window range: unknown flag bits");
  if (first > last || !resident(e, first) || !resident(e, last))
    return fail(e, SA_ERANGE, "window range: first > last or a window of it is not resident");
  return SA_OK;
}

// the engine's own device buffers: the histogram, room for n_keys keys and
// their answers, and the merged registers / summed cells where asked for
int range_buffers(sa_engine *e, uint64_t n_keys, bool regs, bool cells) {
  sa_engine::Range &R = e->range;
  const uint32_t S = e->cfg.n_services;
  if (!R.hist)
    if (int rc = dalloc(e, R.hist, (size_t)S * SA_HLL_HIST_BINS, false, "window range: histogram hipMalloc failed"))
      return rc;
  if (regs && !R.regs)
    if (int rc = dalloc(e, R.regs, e->hll_slot_bytes, false, "window range: register buffer hipMalloc failed")) return rc;
  if (cells && !R.cells)
    if (int rc = dalloc(e, R.cells, e->cms_slot_elems, false, "window range: cell buffer hipMalloc failed")) return rc;
  if (n_keys > R.key_cap) {  // (hipFree waits for the device)
    dfree(e, R.keys);
    R.key_cap = 0;
    const uint64_t want = std::max<uint64_t>(n_keys, 1u << 10);
    if (int rc = dalloc(e, R.keys, want * 2, false, "window range: key buffer hipMalloc failed")) return rc;
    R.key_cap = want;
  }
  return SA_OK;
}

// On `s`: fold_window for every window of first..last, with the windows'
// count folds as one launch (the ERROR slabs of the small rings that have
// them go window by window first)
int range_fold_on(sa_engine *e, uint64_t first, uint64_t last, hipStream_t s) {
  const uint32_t W = e->cfg.n_windows, n = (uint32_t)(last - first + 1);
  for (uint32_t k = 0; k < n; ++k)
    if (int rc = fold_errslab(e, (first + k) & (W - 1), s)) return rc;
  SA_HIP(e, sa::launch_range_fold(e->gkeys, e->errcnt, e->cap, e->cms, e->cms_slot_elems, e->cfg.cms_d, e->cfg.cms_w,
                                  64 - sa::log2u(e->cfg.cms_w), e->d_seeds, e->binned.kinv, e->dense() ? 1u : 0u, W,
                                  first, n, s));
  return SA_OK;
}

// On `s`: every window of first..last folded (its per-slot ERROR counts go to
// its cells before any cell is summed), then the registers max-merged into
// hist (zeroed here) and regs, and the cells summed into cells -- each where
// the pointer is not null.
int range_merge_on(sa_engine *e, uint64_t first, uint64_t last, uint32_t *hist, uint8_t *regs,
                   unsigned long long *cells, hipStream_t s) {
  const uint32_t W = e->cfg.n_windows, n = (uint32_t)(last - first + 1);
  if (int rc = range_fold_on(e, first, last, s)) return rc;
  if (hist) SA_HIP(e, hipMemsetAsync(hist, 0, (size_t)e->cfg.n_services * SA_HLL_HIST_BINS * 4, s));
  if (hist || regs) SA_HIP(e, sa::launch_range_merge(e->hll, W, e->cfg.n_services, e->cfg.hll_p, first, n, hist, regs, s));
  if (cells) SA_HIP(e, sa::launch_range_cells(e->cms, e->cms_slot_elems, W, first, n, cells, s));
  return SA_OK;
}

// From the device arrays to the result, on `s` (waited for): the point
// queries on d_cells, the copies of what the flags ask for, the estimates.
int range_result(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *d_hist, const uint8_t *d_regs,
                 const unsigned long long *d_cells, const uint64_t *keys, uint64_t n_keys, uint32_t flags,
                 hipStream_t s, sa_range_result **out) {
  std::unique_ptr<range_holder> h(new range_holder());
  h->shape(first, last, e->cfg, n_keys, flags);
  hipError_t st = hipSuccess;
  if (n_keys) {
    uint64_t *dk = e->range.keys, *de = dk + e->range.key_cap;
    st = hipMemcpyAsync(dk, keys, n_keys * 8, hipMemcpyHostToDevice, s);
    if (st == hipSuccess)
      st = sa::launch_range_query(d_cells, e->cfg.cms_d, e->cfg.cms_w, 64 - sa::log2u(e->cfg.cms_w), e->d_seeds, dk,
                                  n_keys, reinterpret_cast<unsigned long long *>(de), s);
    if (st == hipSuccess) st = hipMemcpyAsync(h->errors.data(), de, n_keys * 8, hipMemcpyDeviceToHost, s);
  }
  if (st == hipSuccess) st = hipMemcpyAsync(h->hist.data(), d_hist, h->hist.size() * 4, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess && (flags & SA_RANGE_REGISTERS))
    st = hipMemcpyAsync(h->hll.data(), d_regs, h->hll.size(), hipMemcpyDeviceToHost, s);
  if (st == hipSuccess && (flags & SA_RANGE_CELLS))
    st = hipMemcpyAsync(h->cms.data(), d_cells, h->cms.size() * 8, hipMemcpyDeviceToHost, s);
  const hipError_t waited = hipStreamSynchronize(s);  // (also after a failure: a copy into h may be in flight)
  if (st != hipSuccess || waited != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("window range: ") + hipGetErrorString(st != hipSuccess ? st : waited));
  for (uint32_t sv = 0; sv < e->cfg.n_services; ++sv)
    h->distinct[sv] = sa_hll_estimate_hist(h->hist.data() + (size_t)sv * SA_HLL_HIST_BINS, e->cfg.hll_p);
  *out = &h.release()->r;
  return SA_OK;
}

// ---- sliding series (sa_window_series; kernels in spanagg_range.hip) ----
// p (holding cap elements) grown to at least `want`
template <class T>
int series_grow(sa_engine *e, T *&p, uint64_t &cap, uint64_t want, const char *what) {
  if (want <= cap) return SA_OK;
  dfree(e, p);  // (hipFree waits for the device)
  cap = 0;
  if (int rc = dalloc(e, p, want, false, what)) return rc;
  cap = want;
  return SA_OK;
}

int series_buffers(sa_engine *e, uint64_t n_out, uint64_t n_keys) {
  sa_engine::Series &S = e->series;
  if (int rc = series_grow(e, S.hist, S.hist_cap, n_out * e->cfg.n_services * SA_HLL_HIST_BINS,
                           "window series: histogram hipMalloc failed"))
    return rc;
  if (!S.row0)
    if (int rc = dalloc(e, S.row0, e->cfg.n_windows, false, "window series: row sum hipMalloc failed")) return rc;
  if (int rc = series_grow(e, S.keys, S.key_cap, n_keys ? std::max<uint64_t>(n_keys, 1u << 10) : 0,
                           "window series: key buffer hipMalloc failed"))
    return rc;
  return series_grow(e, S.errors, S.err_cap, n_out * n_keys, "window series: answer buffer hipMalloc failed");
}

// ---- heavy hitters (sa_window_top; kernels in spanagg_range.hip) ----
int top_buffers(sa_engine *e) {
  sa_engine::Top &T = e->top;
  if (!T.cand)
    if (int rc = dalloc(e, T.cand, e->cap, false, "window top: candidate buffer hipMalloc failed")) return rc;
  if (!T.ctl)
    if (int rc = dalloc(e, T.ctl, 1, false, "window top: control block hipMalloc failed")) return rc;
  return SA_OK;
}

// On `s`, not waited for: e's key table scanned against d_cells [d][w], the
// first k matches selected and sorted, the counters and k rows copied into *h.
int top_on(sa_engine *e, const unsigned long long *d_cells, uint32_t k, uint64_t min_count, hipStream_t s,
           sa_grp::TopHost *h) {
  const sa_engine::Top &T = e->top;
  try {
    h->rows.resize(k);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window top: the rows do not fit in host memory");
  }
  hipError_t st = sa::launch_top(e->gkeys, e->cap, e->binned.kinv, d_cells, e->cfg.cms_d, e->cfg.cms_w,
                                 64 - sa::log2u(e->cfg.cms_w), e->d_seeds, k, std::max<uint64_t>(min_count, 1), T.cand,
                                 T.ctl, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->head, T.ctl, sizeof h->head, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->rows.data(), T.ctl->sel, (size_t)k * 16, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) return SA_OK;
  (void)hipStreamSynchronize(s);  // (a copy into h may be in flight)
  return fail(e, SA_EDEVICE, std::string("window top: ") + hipGetErrorString(st));
}

// ---- movers (sa_window_movers; kernels in spanagg_range.hip) ----
int movers_buffers(sa_engine *e) {
  if (int rc = top_buffers(e)) return rc;  // (the candidates and the select's state: calls are serialised)
  if (!e->movers.out)
    if (int rc = dalloc(e, e->movers.out, 1, false, "window movers: estimate buffer hipMalloc failed")) return rc;
  return SA_OK;
}

// On `s`, not waited for: e's key table scanned against d_base and d_cur
// [d][w] (the sums of nb and nc windows), the first k matches selected and
// sorted, the counters, the k rows and their estimates copied into *h.
int movers_on(sa_engine *e, const unsigned long long *d_base, const unsigned long long *d_cur, uint64_t nb, uint64_t nc,
              uint32_t k, uint64_t min_score, uint32_t flags, hipStream_t s, sa_grp::MoversHost *h) {
  const sa_engine::Top &T = e->top;
  sa::MoversOut *O = e->movers.out;
  try {
    h->top.rows.resize(k);
    h->out.resize((size_t)k + 1);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window movers: the rows do not fit in host memory");
  }
  hipError_t st = sa::launch_movers(e->gkeys, e->cap, e->binned.kinv, d_base, d_cur, e->cfg.cms_d, e->cfg.cms_w,
                                    64 - sa::log2u(e->cfg.cms_w), e->d_seeds, nb, nc, flags & SA_MOVERS_FALL ? 1u : 0u, k,
                                    std::max<uint64_t>(min_score, 1), T.cand, T.ctl, O, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->top.head, T.ctl, sizeof h->top.head, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->top.rows.data(), T.ctl->sel, (size_t)k * 16, hipMemcpyDeviceToHost, s);
  // (MoversOut: the 16-byte head, then the rows)
  if (st == hipSuccess) st = hipMemcpyAsync(h->out.data(), O, ((size_t)k + 1) * 16, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) return SA_OK;
  (void)hipStreamSynchronize(s);  // (a copy into h may be in flight)
  return fail(e, SA_EDEVICE, std::string("window movers: ") + hipGetErrorString(st));
}

// ---- service overlap (sa_window_overlap; kernels in spanagg_range.hip and spanagg_overlap.hip) ----
// The counting form of the pair kernel: the laboratory build reads
// SPANAGG_OVERLAP (0, 1, 2) at every call, the product holds variant 0 alone.
uint32_t overlap_variant() {
#ifdef SPANAGG_AB
  if (const char *v = ab_env("SPANAGG_OVERLAP")) return (uint32_t)std::atoi(v);
#endif
  return 0;
}

int overlap_buffers(sa_engine *e) {
  sa_engine::Overlap &O = e->overlap;
  const size_t cap = std::min<size_t>(e->cfg.n_services, SA_OVERLAP_MAX_SERVICES);
  if (!O.map)
    if (int rc = dalloc(e, O.map, cap, false, "window overlap: selection hipMalloc failed")) return rc;
  if (!O.hist)
    if (int rc = dalloc(e, O.hist, cap * SA_HLL_HIST_BINS, false, "window overlap: histogram hipMalloc failed")) return rc;
  if (!O.pair_hist)
    if (int rc = dalloc(e, O.pair_hist, cap * (cap - 1) / 2 * SA_HLL_HIST_BINS, false,
                        "window overlap: pair histogram hipMalloc failed"))
      return rc;
  if (!O.regs)
    if (int rc = dalloc(e, O.regs, cap << e->cfg.hll_p, false, "window overlap: register buffer hipMalloc failed"))
      return rc;
  return SA_OK;
}

// On `s` (waited for): the registers regs [n_win slots of n_services][2^p] of
// windows first .. first + n_win - 1 (ring of n_windows slots) max-merged for
// the services of sel, their histograms, the pairs' histograms, the copies
// into the result and the estimates.
int overlap_on(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *regs, uint32_t n_windows, uint64_t from,
               uint32_t n_win, const std::vector<uint32_t> &sel, hipStream_t s, sa_overlap_result **out) {
  std::unique_ptr<overlap_holder> h;
  try {
    h.reset(new overlap_holder());
    h->shape(first, last, sel, e->cfg.hll_p);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window overlap: the result does not fit in host memory");
  }
  if (int rc = overlap_buffers(e)) return rc;
  const sa_engine::Overlap &O = e->overlap;
  const uint32_t n = (uint32_t)sel.size(), p = e->cfg.hll_p;
  hipError_t st = hipMemcpyAsync(O.map, sel.data(), (size_t)n * 4, hipMemcpyHostToDevice, s);
  if (st == hipSuccess) st = hipMemsetAsync(O.hist, 0, h->hist.size() * 4, s);
  if (st == hipSuccess && h->r.n_pairs) st = hipMemsetAsync(O.pair_hist, 0, h->pair_hist.size() * 4, s);
  if (st == hipSuccess)
    st = sa::launch_range_merge_sel(regs, n_windows, e->cfg.n_services, p, from, n_win, O.map, n, O.hist, O.regs, s);
  if (st == hipSuccess) st = sa::launch_overlap_pairs(O.regs, n, p, O.pair_hist, overlap_variant(), s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->hist.data(), O.hist, h->hist.size() * 4, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess && h->r.n_pairs)
    st = hipMemcpyAsync(h->pair_hist.data(), O.pair_hist, h->pair_hist.size() * 4, hipMemcpyDeviceToHost, s);
  const hipError_t waited = hipStreamSynchronize(s);  // the call's one wait (also after a failure: copies may be in flight)
  if (st != hipSuccess || waited != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("window overlap: ") + hipGetErrorString(st != hipSuccess ? st : waited));
  for (uint32_t i = 0; i < n; ++i)
    h->distinct[i] = sa_hll_estimate_hist(h->hist.data() + (size_t)i * SA_HLL_HIST_BINS, p);
  size_t pair = 0;
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t j = i + 1; j < n; ++j, ++pair) {
      h->union_est[pair] = sa_hll_estimate_hist(h->pair_hist.data() + pair * SA_HLL_HIST_BINS, p);
      h->shared[pair] = std::fmax(0.0, (h->distinct[i] + h->distinct[j]) - h->union_est[pair]);
    }
  *out = &h.release()->r;
  return SA_OK;
}
// ---- latency quantiles (sa_window_latency; kernels in spanagg_latency.hip) ----
// rows of sliding sums one tile of outputs holds (64 MiB; at least one output's)
constexpr uint64_t kLatTileRows = 1u << 15;

int latency_enabled(sa_engine *e) {
  if (e->lat.ring) return SA_OK;
  return fail(e, SA_ESTATE, "window latency: the engine was not created with SA_OPT_WINDOW_LATENCY");
}

int latency_range(sa_engine *e, uint64_t first, uint64_t last, uint32_t width) {
  if (first > last || width == 0 || width > e->cfg.n_windows || first + 1 < width || !resident(e, first - width + 1) ||
      !resident(e, last))
    return fail(e, SA_ERANGE, "window latency: first > last, a width outside 1..n_windows, or a covered window is not resident");
  return SA_OK;
}

// Room for a selection of n_sel ids, sum_rows rows of sliding sums in the
// engine's own tile and `rows` rows' counts and quantile bins.
int latency_buffers(sa_engine *e, uint64_t n_sel, uint64_t sum_rows, uint64_t rows, uint32_t n_q) {
  sa_engine::Latency &L = e->lat;
  if (int rc = series_grow(e, L.sel, L.sel_cap, n_sel ? std::max<uint64_t>(n_sel, 64) : 0,
                           "window latency: selection hipMalloc failed"))
    return rc;
  if (int rc = series_grow(e, L.sums, L.sums_cap, sum_rows * SA_LAT_BINS, "window latency: sum buffer hipMalloc failed"))
    return rc;
  if (int rc = series_grow(e, L.count, L.row_cap, rows, "window latency: count buffer hipMalloc failed")) return rc;
  return series_grow(e, L.q_bin, L.qbin_cap, rows * n_q, "window latency: quantile buffer hipMalloc failed");
}

// A member's part of a group query on `s`: the selection onto the device and
// the sums stage behind it, sums [n_out][sel.size()][SA_LAT_BINS] from window
// `a` on.  The copy reads the caller's pageable `sel` asynchronously, so it is
// queued after everything that can fail without a wait, and a failure behind
// it waits for `s` before it returns; on success the group waits before `sel` goes.
hipError_t latency_sums_on(sa_engine *e, const std::vector<uint32_t> &sel, uint64_t a, uint32_t width, uint32_t n_out,
                           unsigned long long *d_sums, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  hipError_t st = hipMemcpyAsync(L.sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s);
  if (st == hipSuccess)
    st = sa::launch_lat_sums(L.ring, e->cfg.n_services, e->cfg.n_windows, L.sel, (uint32_t)sel.size(), a, width, n_out,
                             d_sums, s);
  if (st != hipSuccess) (void)hipStreamSynchronize(s);
  return st;
}

// On `s`: the counts and quantile bins of rows row0 .. row0 + n_rows - 1 from
// their sums d_sums [n_rows][SA_LAT_BINS], and with SA_LAT_HIST the sums' copy
// into the result.
hipError_t latency_scan_on(sa_engine *e, const unsigned long long *d_sums, uint64_t row0, uint64_t n_rows,
                           latency_holder *h, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  const uint32_t n_q = h->r.n_q;
  hipError_t st = sa::launch_lat_scan(d_sums, n_rows, h->q_ppm.data(), n_q, L.count + row0, L.q_bin + row0 * n_q, s);
  if (st == hipSuccess && h->r.hist)
    st = hipMemcpyAsync(h->hist.data() + row0 * SA_LAT_BINS, d_sums, n_rows * SA_LAT_BINS * 8, hipMemcpyDeviceToHost, s);
  return st;
}

// The counts and bins into the result (st: what the launches before returned),
// the call's one wait -- also after a failure: a copy into h may be in flight
// -- and every bin's upper bound.
int latency_collect(sa_engine *e, hipError_t st, std::unique_ptr<latency_holder> &h, hipStream_t s,
                    sa_latency_result **out) {
  const sa_engine::Latency &L = e->lat;
  if (st == hipSuccess) st = hipMemcpyAsync(h->count.data(), L.count, h->count.size() * 8, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->q_bin.data(), L.q_bin, h->q_bin.size(), hipMemcpyDeviceToHost, s);
  const hipError_t waited = hipStreamSynchronize(s);
  if (st != hipSuccess || waited != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("window latency: ") + hipGetErrorString(st != hipSuccess ? st : waited));
  const uint32_t n_q = h->r.n_q;
  for (size_t row = 0; row < h->count.size(); ++row)
    for (uint32_t i = 0; i < n_q; ++i) {
      uint64_t lo = 0, hi = 0;
      if (h->count[row]) (void)sa_latency_bin_bounds(h->q_bin[row * n_q + i], &lo, &hi);
      h->q_ns[row * n_q + i] = hi;
    }
  *out = &h.release()->r;
  return SA_OK;
}

std::unique_ptr<latency_holder> latency_result(sa_engine *e, uint64_t first, uint64_t last, uint32_t width,
                                               const std::vector<uint32_t> &sel, const uint32_t *q_ppm, uint32_t n_q,
                                               uint32_t flags) {
  std::unique_ptr<latency_holder> h;
  try {
    h.reset(new latency_holder());
    h->shape(first, last, width, sel, q_ppm, n_q, flags);
  } catch (const std::bad_alloc &) {
    h.reset();
    (void)fail(e, SA_ENOMEM, "window latency: the result does not fit in host memory");
  }
  return h;
}

// ---- latency movers (sa_window_latency_movers; kernels in spanagg_latency.hip, the select in spanagg_range.hip) ----
// range: base first, base last, current first, current last
int latency_movers_ranges(sa_engine *e, const uint64_t range[4]) {
  for (int i = 0; i < 4; i += 2)
    if (range[i] > range[i + 1] || !resident(e, range[i]) || !resident(e, range[i + 1]))
      return fail(e, SA_ERANGE, "window latency movers: first > last or a window of a range is not resident");
  return SA_OK;
}

// Both ranges' sums of the engine's own ring [2][n_services][SA_LAT_BINS].
int latency_movers_sums(sa_engine *e) {
  sa_engine::Latency &L = e->lat;
  if (L.mov_sums) return SA_OK;
  return dalloc(e, L.mov_sums, 2 * (size_t)e->cfg.n_services * SA_LAT_BINS, false,
                "window latency movers: sum buffer hipMalloc failed");
}

// What the stages after the sums work in: the counts, the candidates (one a
// service), the rows, and sa_window_top's control block.
int latency_movers_buffers(sa_engine *e) {
  sa_engine::Latency &L = e->lat;
  const size_t S = e->cfg.n_services;
  if (!e->top.ctl)
    if (int rc = dalloc(e, e->top.ctl, 1, false, "window latency movers: control block hipMalloc failed")) return rc;
  if (!L.mov_counts)
    if (int rc = dalloc(e, L.mov_counts, 2 * S, false, "window latency movers: count buffer hipMalloc failed")) return rc;
  if (!L.mov_cand)
    if (int rc = dalloc(e, L.mov_cand, S, false, "window latency movers: candidate buffer hipMalloc failed")) return rc;
  if (!L.mov_out)
    if (int rc = dalloc(e, L.mov_out, 1, false, "window latency movers: row buffer hipMalloc failed")) return rc;
  return SA_OK;
}

hipError_t latency_movers_sums_on(sa_engine *e, const uint64_t range[4], unsigned long long *d_sums, hipStream_t s) {
  return sa::launch_lat_pair_sums(e->lat.ring, e->cfg.n_services, e->cfg.n_windows, range[0],
                                  (uint32_t)(range[1] - range[0] + 1), range[2], (uint32_t)(range[3] - range[2] + 1),
                                  d_sums, s);
}
}  // namespace

namespace sa_grp {
const char *latency_args(uint32_t n_services, const uint32_t *services, uint32_t n_sel, const uint32_t *q_ppm,
                         uint32_t n_q, uint32_t flags, std::vector<uint32_t> *sel) {
  sel->clear();
  if (flags & ~SA_LAT_HIST) return "window latency: unknown flag bits";
  if (n_q == 0 || n_q > SA_LAT_MAX_Q || !q_ppm) return "window latency: n_q outside 1..SA_LAT_MAX_Q or null q_ppm";
  for (uint32_t i = 0; i < n_q; ++i)
    if (q_ppm[i] == 0 || q_ppm[i] > 1000000u) return "window latency: a q_ppm outside 1..1000000";
  if (!services) {
    if (n_sel) return "window latency: n_sel != 0 with null services";
    for (uint32_t i = 0; i < n_services; ++i) sel->push_back(i);
    return nullptr;
  }
  if (n_sel == 0) return "window latency: an empty selection";
  if (n_sel > n_services) return "window latency: more ids than services (a repeated id)";
  std::vector<bool> seen(n_services, false);
  for (uint32_t i = 0; i < n_sel; ++i) {
    if (services[i] >= n_services) return "window latency: a service id at or past n_services";
    if (seen[services[i]]) return "window latency: a repeated service id";
    seen[services[i]] = true;
    sel->push_back(services[i]);
  }
  return nullptr;
}

const char *latency_rows(uint64_t n_out, uint64_t n_sel, uint32_t flags) {
  if (n_out * n_sel > ((flags & SA_LAT_HIST) ? 1ull << 16 : 1ull << 20))
    return "window latency: n_out * n_sel above 2^20 (2^16 with SA_LAT_HIST)";
  return nullptr;
}

int window_latency_export_async(sa_engine *e, uint64_t first, uint64_t last, uint32_t width,
                                const std::vector<uint32_t> &sel, uint64_t *d_sums, hipStream_t s) {
  if (!e || !d_sums || sel.empty()) return SA_EINVAL;
  if (int rc = latency_enabled(e)) return rc;
  if (int rc = latency_range(e, first, last, width)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = latency_buffers(e, sel.size(), 0, 0, 0)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, latency_sums_on(e, sel, first - width + 1, width, (uint32_t)(last - first + 1),
                            reinterpret_cast<unsigned long long *>(d_sums), s));
  if (int rc = hop_back(e, s)) {  // (the selection buffer is the engine's)
    (void)hipStreamSynchronize(s);
    return rc;
  }
  return SA_OK;
}

int window_latency_finish(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const std::vector<uint32_t> &sel,
                          const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, const uint64_t *d_sums, hipStream_t s,
                          sa_latency_result **out) {
  if (!e || !out || !d_sums || sel.empty()) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  std::unique_ptr<latency_holder> h = latency_result(e, first, last, width, sel, q_ppm, n_q, flags);
  if (!h) return SA_ENOMEM;
  const uint64_t rows = h->count.size();
  if (int rc = latency_buffers(e, 0, 0, rows, n_q)) return rc;
  const hipError_t st = latency_scan_on(e, reinterpret_cast<const unsigned long long *>(d_sums), 0, rows, h.get(), s);
  return latency_collect(e, st, h, s, out);
}

const char *latency_movers_args(uint32_t k, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags) {
  if (k == 0 || k > SA_TOP_MAX_K) return "window latency movers: k outside 1..SA_TOP_MAX_K";
  if (flags & ~SA_LATMOV_FALL) return "window latency movers: unknown flag bits";
  if (n_q == 0 || n_q > SA_LAT_MAX_Q || !q_ppm) return "window latency movers: n_q outside 1..SA_LAT_MAX_Q or null q_ppm";
  for (uint32_t i = 0; i < n_q; ++i)
    if (q_ppm[i] == 0 || q_ppm[i] > 1000000u) return "window latency movers: a q_ppm outside 1..1000000";
  return nullptr;
}

int window_latency_movers_export_async(sa_engine *e, const uint64_t range[4], uint64_t *d_sums, hipStream_t s) {
  if (!e || !d_sums) return SA_EINVAL;
  if (int rc = latency_enabled(e)) return rc;
  if (int rc = latency_movers_ranges(e, range)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, latency_movers_sums_on(e, range, reinterpret_cast<unsigned long long *>(d_sums), s));
  return hop_back(e, s);  // (a later launch that writes the ring orders after these reads)
}

int window_latency_movers_finish(sa_engine *e, const uint64_t range[4], uint32_t k, uint64_t min_count,
                                 uint32_t min_shift, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                                 const uint64_t *d_sums, hipStream_t s, sa_latency_movers_result **out) {
  if (!e || !out || !d_sums) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = latency_movers_buffers(e)) return rc;
  const sa_engine::Latency &L = e->lat;
  sa::TopCtl *T = e->top.ctl;
  unsigned long long head[4] = {};
  std::vector<ulonglong2> sel;
  std::vector<unsigned char> rows;  // LatMovOut's head and its first k rows
  try {
    sel.resize(k);
    rows.resize(offsetof(sa::LatMovOut, row) + (size_t)k * sizeof(sa::LatMovRow));
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency movers: the rows do not fit in host memory");
  }
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  hipError_t st = sa::launch_lat_movers(reinterpret_cast<const unsigned long long *>(d_sums), e->cfg.n_services, k,
                                        std::max<uint64_t>(min_count, 1), std::max(min_shift, 1u),
                                        flags & SA_LATMOV_FALL ? 1u : 0u, q_ppm, n_q, L.mov_counts, L.mov_cand, T,
                                        L.mov_out, s);
  if (st == hipSuccess) st = hipMemcpyAsync(head, T, sizeof head, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(sel.data(), T->sel, (size_t)k * 16, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(rows.data(), L.mov_out, rows.size(), hipMemcpyDeviceToHost, s);
  const hipError_t waited = hipStreamSynchronize(s);  // the call's one wait (also after a failure: copies may be in flight)
  if (st != hipSuccess || waited != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("window latency movers: ") + hipGetErrorString(st != hipSuccess ? st : waited));
  const uint32_t n = (uint32_t)std::min<uint64_t>(k, head[0]);
  std::unique_ptr<latency_movers_holder> h;
  try {
    h.reset(new latency_movers_holder());
    h->shape(range, k, n, q_ppm, n_q, flags, e->cfg.n_services);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency movers: the result does not fit in host memory");
  }
  // (TopCtl's head: the matches, the eligible services, ..; LatMovOut's: the two ranges' spans)
  h->r.n_matched = head[0], h->r.n_eligible = head[1];
  std::memcpy(&h->r.spans_base, rows.data(), 8);
  std::memcpy(&h->r.spans_cur, rows.data() + 8, 8);
  for (uint32_t i = 0; i < n; ++i) {
    sa::LatMovRow row;
    std::memcpy(&row, rows.data() + offsetof(sa::LatMovOut, row) + (size_t)i * sizeof row, sizeof row);
    h->services[i] = (uint32_t)sel[i].y;
    h->shift[i] = (int32_t)(sel[i].x >> 48);
    h->count_base[i] = row.count[0], h->count_cur[i] = row.count[1];
    for (uint32_t q = 0; q < n_q; ++q) {
      uint64_t lo = 0, hi = 0;
      const size_t at = (size_t)i * n_q + q;
      h->q_bin_base[at] = row.q_bin[0][q], h->q_bin_cur[at] = row.q_bin[1][q];
      // (a returned row is eligible: neither count is 0)
      (void)sa_latency_bin_bounds(row.q_bin[0][q], &lo, &hi);
      h->q_ns_base[at] = row.count[0] ? hi : 0;
      (void)sa_latency_bin_bounds(row.q_bin[1][q], &lo, &hi);
      h->q_ns_cur[at] = row.count[1] ? hi : 0;
    }
  }
  *out = &h.release()->r;
  return SA_OK;
}

const char *overlap_select(uint32_t n_services, const uint32_t *services, uint32_t n_sel, std::vector<uint32_t> *sel) {
  sel->clear();
  if (!services) {
    if (n_sel) return "window overlap: n_sel != 0 with null services";
    if (n_services > SA_OVERLAP_MAX_SERVICES)
      return "window overlap: every service asked for on an engine with more than SA_OVERLAP_MAX_SERVICES";
    for (uint32_t i = 0; i < n_services; ++i) sel->push_back(i);
    return nullptr;
  }
  if (n_sel == 0) return "window overlap: an empty selection";
  if (n_sel > SA_OVERLAP_MAX_SERVICES) return "window overlap: more than SA_OVERLAP_MAX_SERVICES services";
  for (uint32_t i = 0; i < n_sel; ++i) {
    if (services[i] >= n_services) return "window overlap: a service id at or past n_services";
    if (std::find(sel->begin(), sel->end(), services[i]) != sel->end()) return "window overlap: a repeated service id";
    sel->push_back(services[i]);
  }
  return nullptr;
}

int window_overlap_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, hipStream_t s) {
  if (!e || !d_hll) return SA_EINVAL;
  if (int rc = range_args(e, first, last, nullptr, 0, 0)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, sa::launch_range_merge(e->hll, e->cfg.n_windows, e->cfg.n_services, e->cfg.hll_p, first,
                                   (uint32_t)(last - first + 1), nullptr, d_hll, s));
  return hop_back(e, s);
}

int window_overlap_finish(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *d_hll,
                          const std::vector<uint32_t> &sel, hipStream_t s, sa_overlap_result **out) {
  if (!e || !out || !d_hll || sel.empty()) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  // (the merged array as a ring of one window: the gather of the selected rows)
  return overlap_on(e, first, last, d_hll, 1, 0, 1, sel, s, out);
}

bool over_reclaim_threshold(const sa_engine *e, uint64_t nk) {
  return sa::binned_like(e->path) ? 20 * nk > 7 * (uint64_t)e->cap : 2 * nk > e->cap;
}

int export_keys_async(sa_engine *e, uint64_t *d_keys, uint64_t cap, uint64_t *h_n, uint64_t *h_dropped,
                      hipStream_t s) {
  if (!e || !h_n || !h_dropped || (cap && !d_keys)) return SA_EINVAL;
  if (sa::expo_like(e->path)) return fail(e, SA_ESTATE, "merge hooks cover explicit-bucket engines only");
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;  // (the group's member stream, never the engine's own)
  if (int rc = export_keys_on(e, d_keys, cap, s)) return rc;
  SA_HIP(e, hipMemcpyAsync(h_n, e->scratch, 8, hipMemcpyDeviceToHost, s));
  SA_HIP(e, hipMemcpyAsync(h_dropped, e->stats + sa::kStatDropped, 8, hipMemcpyDeviceToHost, s));
  return hop_back(e, s);  // later engine work (the gather's counter reset) orders after these reads
}

int count_keys_async(sa_engine *e, uint64_t *h_n) {
  if (!e || !h_n) return SA_EINVAL;
  if (int rc = begin_read(e)) return rc;
  return count_keys(e, h_n, 1);
}

int reclaim_async(sa_engine *e) {
  if (!e) return SA_EINVAL;
  if (e->unflushed) return fail(e, SA_ESTATE, "reclaim: spans ingested since the last flush");
  if (int rc = set_dev(e)) return rc;
  return reclaim_now(e);
}

uint64_t table_capacity(const sa_engine *e) { return e ? e->cap : 0; }

int sync_stream(sa_engine *e) {
  if (!e) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));
  return SA_OK;
}

int window_range_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, uint64_t *d_cms,
                              hipStream_t s) {
  if (!e || !d_cms) return SA_EINVAL;
  if (int rc = range_args(e, first, last, nullptr, 0, 0)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = range_merge_on(e, first, last, nullptr, d_hll, reinterpret_cast<unsigned long long *>(d_cms), s))
    return rc;
  return hop_back(e, s);  // (the folds wrote this engine's cells and ERROR counts)
}

int window_range_finish(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *d_hll, const uint64_t *d_cms,
                        const uint64_t *keys, uint64_t n_keys, uint32_t flags, hipStream_t s, sa_range_result **out) {
  if (!e || !out || !d_hll || !d_cms) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = range_buffers(e, n_keys, false, false)) return rc;  // (the merged arrays are the group's)
  uint32_t *hist = e->range.hist;
  SA_HIP(e, hipMemsetAsync(hist, 0, (size_t)e->cfg.n_services * SA_HLL_HIST_BINS * 4, s));
  SA_HIP(e, sa::launch_hll_hist(d_hll, e->cfg.n_services, e->cfg.hll_p, hist, s));
  return range_result(e, first, last, hist, d_hll, reinterpret_cast<const unsigned long long *>(d_cms), keys, n_keys,
                      flags, s, out);
}

int window_top_async(sa_engine *e, const uint64_t *d_cms, uint32_t k, uint64_t min_count, hipStream_t s, TopHost *out) {
  if (!e || !d_cms || !out) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = top_buffers(e)) return rc;
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = top_on(e, reinterpret_cast<const unsigned long long *>(d_cms), k, min_count, s, out)) return rc;
  return hop_back(e, s);
}

int window_movers_async(sa_engine *e, const uint64_t *d_base, const uint64_t *d_cur, uint64_t nb, uint64_t nc,
                        uint32_t k, uint64_t min_score, uint32_t flags, hipStream_t s, MoversHost *out) {
  if (!e || !d_base || !d_cur || !out) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = movers_buffers(e)) return rc;
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = movers_on(e, reinterpret_cast<const unsigned long long *>(d_base),
                         reinterpret_cast<const unsigned long long *>(d_cur), nb, nc, k, min_score, flags, s, out))
    return rc;
  return hop_back(e, s);
}

namespace {
// A row of a ranked answer: its key, what it is ranked by, and what travels
// with it (sa_window_movers: the two estimates).
struct Ranked {
  uint64_t key, rank, a, b;
  bool operator<(const Ranked &o) const { return std::tie(key, rank, a, b) < std::tie(o.key, o.rank, o.a, o.b); }
  bool operator==(const Ranked &o) const { return std::tie(key, rank, a, b) == std::tie(o.key, o.rank, o.a, o.b); }
};

// The answer of n scans (each waited for; member j's first min(k, head[0])
// rows, extra[j] the values that travel with them or nullptr): one member's
// rows as they are, the device's order; several members' merged -- a series on
// several members has the same row on each: once -- by (rank descending, key
// ascending), cut to k.
std::vector<Ranked> ranked_rows(uint32_t k, const TopHost *const *m, const ulonglong2 *const *extra, uint32_t n) {
  std::vector<Ranked> all;
  for (uint32_t j = 0; j < n; ++j) {
    const size_t rows = (size_t)std::min<uint64_t>(k, m[j]->head[0]);
    for (size_t i = 0; i < rows; ++i)
      all.push_back(Ranked{m[j]->rows[i].y, m[j]->rows[i].x, extra[j] ? extra[j][i].x : 0, extra[j] ? extra[j][i].y : 0});
  }
  if (n == 1) return all;
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  std::sort(all.begin(), all.end(),
            [](const Ranked &a, const Ranked &b) { return a.rank != b.rank ? a.rank > b.rank : a.key < b.key; });
  if (all.size() > k) all.resize(k);
  return all;
}
}  // namespace

int top_result(uint64_t first, uint64_t last, uint32_t k, const TopHost *m, uint32_t n_members, sa_top_result **out) {
  try {
    std::unique_ptr<top_holder> h(new top_holder());
    std::vector<const TopHost *> tops(n_members);
    for (uint32_t j = 0; j < n_members; ++j) tops[j] = &m[j];
    const std::vector<const ulonglong2 *> none(n_members, nullptr);
    const std::vector<Ranked> rows = ranked_rows(k, tops.data(), none.data(), n_members);
    h->shape(first, last, k, (uint32_t)rows.size());
    for (size_t i = 0; i < rows.size(); ++i) h->keys[i] = rows[i].key, h->errors[i] = rows[i].rank;
    for (uint32_t j = 0; j < n_members; ++j) h->r.n_matched += m[j].head[0], h->r.n_resident += m[j].head[1];
    h->r.error_spans = m[0].head[3];  // (the merged cells are the same on every member)
    *out = &h.release()->r;
    return SA_OK;
  } catch (const std::bad_alloc &) {
    return SA_ENOMEM;
  }
}

int movers_result(const uint64_t range[4], uint32_t k, uint32_t flags, const MoversHost *m, uint32_t n_members,
                  sa_movers_result **out) {
  try {
    std::unique_ptr<movers_holder> h(new movers_holder());
    std::vector<const TopHost *> tops(n_members);
    std::vector<const ulonglong2 *> est(n_members);
    for (uint32_t j = 0; j < n_members; ++j) tops[j] = &m[j].top, est[j] = m[j].out.data() + 1;
    const std::vector<Ranked> rows = ranked_rows(k, tops.data(), est.data(), n_members);
    h->shape(range, k, (uint32_t)rows.size(), flags);
    for (size_t i = 0; i < rows.size(); ++i) {
      h->keys[i] = rows[i].key, h->score[i] = (int64_t)rows[i].rank;  // (a match's score is >= 1)
      h->baseline[i] = rows[i].a, h->current[i] = rows[i].b;
    }
    for (uint32_t j = 0; j < n_members; ++j) h->r.n_matched += m[j].top.head[0], h->r.n_resident += m[j].top.head[1];
    // (the merged cells are the same on every member)
    h->r.error_spans_base = m[0].out[0].x, h->r.error_spans_cur = m[0].top.head[3];
    *out = &h.release()->r;
    return SA_OK;
  } catch (const std::bad_alloc &) {
    return SA_ENOMEM;
  }
}
}  // namespace sa_grp

extern "C" {

int sa_reclaim_keys(sa_engine *e, int force) {
  if (!e) return SA_EINVAL;
  if (e->dense()) return fail(e, SA_ESTATE, "sa_reclaim_keys: dense-index engine (the host recycles indices with sa_bind_ids)");
  if (e->unflushed) return fail(e, SA_ESTATE, "sa_reclaim_keys: spans ingested since the last flush");
  if (int rc = begin_read(e)) return rc;
  if (int rc = force ? reclaim_now(e) : reclaim_if_full(e)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));
  return SA_OK;
}

int sa_flush(sa_engine *e, sa_red_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (sa::expo_like(e->path)) return fail(e, SA_ESTATE, "exponential-histogram engine: use sa_flush_exp");
  if (int rc = begin_read(e)) return rc;
  const uint32_t nbk = e->hist.nbk, stride = nbk + 1;
  if (!e->out_keys && (dalloc(e, e->out_keys, e->cap, false) || dalloc(e, e->out_rows, e->cap * stride, false)))
    return fail(e, SA_ENOMEM, "flush buffers hipMalloc failed");
  if (int rc = reduce_slabs(e, e->stream)) return rc;
  SA_HIP(e, hipMemsetAsync(e->scratch, 0, 8, e->stream));
  SA_HIP(e, sa::launch_compact(e->gkeys, e->gcounts, e->cap, geom(e), e->out_keys, e->out_rows,
                               e->scratch, e->cap, 1, e->stream));
  uint64_t n = 0;
  SA_HIP(e, hipMemcpyAsync(&n, e->scratch, 8, hipMemcpyDeviceToHost, e->stream));
  SA_HIP(e, hipStreamSynchronize(e->stream));
  std::vector<uint64_t> k(n), rows(n * stride);
  if (n) {
    SA_HIP(e, hipMemcpyAsync(k.data(), e->out_keys, n * 8, hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipMemcpyAsync(rows.data(), e->out_rows, n * stride * 8, hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipStreamSynchronize(e->stream));
  }
  const std::vector<uint64_t> ord = key_order(k);
  auto *h = new red_holder();
  h->shape(n, nbk);
  const double div = unit_div(e);
  for (uint64_t r = 0; r < n; ++r) {
    const uint64_t i = ord[r];
    h->keys[r] = k[i];
    uint64_t c = 0;
    for (uint32_t b = 0; b < nbk; ++b) {
      h->counts[r * nbk + b] = rows[i * stride + b];
      c += rows[i * stride + b];
    }
    h->calls[r] = c;
    h->sum_ns[r] = rows[i * stride + nbk];
    h->sum[r] = (double)h->sum_ns[r] / div;
  }
  *out = &h->r;
  return finish_flush(e);
}

void sa_red_result_free(sa_red_result *r) { delete reinterpret_cast<red_holder *>(r); }

int sa_flush_exp(sa_engine *e, sa_exp_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (!sa::expo_like(e->path)) return fail(e, SA_ESTATE, "explicit-bucket engine: use sa_flush");
  if (int rc = begin_read(e)) return rc;
  sa_engine::Expo &x = e->expo;
  const uint32_t M = e->cfg.exp_max_size;
  if (!x.out_keys && (dalloc(e, x.out_keys, e->cap, false) || dalloc(e, x.out_rows, e->cap, false) ||
                      dalloc(e, x.out_buckets, e->cap * (size_t)M, false)))
    return fail(e, SA_ENOMEM, "expo flush buffers hipMalloc failed");
  SA_HIP(e, hipMemsetAsync(e->scratch, 0, 8, e->stream));
  SA_HIP(e, sa::launch_expo_compact(expo_params(e, nullptr), x.out_keys, x.out_rows, x.out_buckets, e->scratch,
                                    e->stream));
  uint64_t n = 0;
  SA_HIP(e, hipMemcpyAsync(&n, e->scratch, 8, hipMemcpyDeviceToHost, e->stream));
  SA_HIP(e, hipStreamSynchronize(e->stream));
  std::vector<uint64_t> k(n);
  std::vector<sa::ExpoRow> rows(n);
  std::vector<uint32_t> bk(n * M);
  if (n) {
    SA_HIP(e, hipMemcpyAsync(k.data(), x.out_keys, n * 8, hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipMemcpyAsync(rows.data(), x.out_rows, n * sizeof(sa::ExpoRow), hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipMemcpyAsync(bk.data(), x.out_buckets, n * (size_t)M * 4, hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipStreamSynchronize(e->stream));
  }
  const std::vector<uint64_t> ord = key_order(k);
  auto *h = new exp_holder();
  h->shape(n, M, e->cfg.unit);
  const double div = unit_div(e);
  for (uint64_t r = 0; r < n; ++r) {
    const uint64_t i = ord[r];
    const sa::ExpoRow &row = rows[i];
    h->keys[r] = k[i];
    h->count[r] = row.count;
    h->zero[r] = row.zero;
    h->sum_ns[r] = row.sum_ns;
    h->sum[r] = (double)row.sum_ns / div;
    h->min[r] = (double)row.min_ns / div;
    h->max[r] = (double)row.max_ns / div;
    h->scale[r] = row.scale;
    h->offset[r] = row.offset;
    h->nb[r] = row.n;
    for (uint32_t j = 0; j < row.n && j < M; ++j) h->buckets[r * M + j] = bk[i * M + j];
  }
  *out = &h->r;
  return finish_flush(e);
}

void sa_exp_result_free(sa_exp_result *r) { delete reinterpret_cast<exp_holder *>(r); }

int sa_expo_probe(sa_engine *e, const double *v, const int32_t *scale, uint64_t n, int32_t *out, double *logs) {
  if (!e || (n && (!v || !scale || !out || !logs)) || n > (1ULL << 20)) return SA_EINVAL;
  if (n == 0) return SA_OK;
  if (int rc = begin_read(e)) return rc;
  char *buf = nullptr;
  if (int rc = dalloc(e, buf, n * 24, false, "probe buffer")) return rc;
  double *dv = reinterpret_cast<double *>(buf), *dl = dv + n;
  int32_t *ds = reinterpret_cast<int32_t *>(dl + n), *di = ds + n;
  hipError_t st = hipMemcpyAsync(dv, v, n * 8, hipMemcpyHostToDevice, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(ds, scale, n * 4, hipMemcpyHostToDevice, e->stream);
  if (st == hipSuccess) st = sa::launch_expo_probe(dv, ds, di, dl, n, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(out, di, n * 4, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(logs, dl, n * 8, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  dfree(e, buf);
  return st == hipSuccess ? SA_OK : fail(e, SA_EDEVICE, std::string("expo probe: ") + hipGetErrorString(st));
}

int sa_key_union_probe(sa_engine *e, const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *n_out) {
  if (!e || !n_out || (n && (!in || !out)) || n > (1ULL << 28)) return SA_EINVAL;
  *n_out = 0;
  if (n == 0) return SA_OK;
  if (int rc = begin_read(e)) return rc;
  char *buf = nullptr;
  const size_t scratch = sa::key_union_scratch_bytes(n);
  if (int rc = dalloc(e, buf, n * 16 + scratch + 64, false, "probe buffer")) return rc;
  auto *din = reinterpret_cast<uint64_t *>(buf), *dout = din + n;
  auto *dtot = reinterpret_cast<uint32_t *>(dout + n);
  void *dscr = reinterpret_cast<char *>(dtot) + 64;
  uint64_t *big = nullptr;  // (key_union's own allocation: freed here)
  size_t big_bytes = 0;
  uint32_t tot = 0;
  hipError_t st = hipMemcpyAsync(din, in, n * 8, hipMemcpyHostToDevice, e->stream);
  if (st == hipSuccess) st = sa::key_union(din, n, dout, dtot, dscr, &big, &big_bytes, e->stream);
  if (st == hipSuccess) st = hipMemcpyAsync(&tot, dtot, 4, hipMemcpyDeviceToHost, e->stream);
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  if (st == hipSuccess && tot) st = hipMemcpy(out, dout, (size_t)tot * 8, hipMemcpyDeviceToHost);
  if (big) (void)hipFree(big);
  dfree(e, buf);
  if (st != hipSuccess) return fail(e, SA_EDEVICE, std::string("key union probe: ") + hipGetErrorString(st));
  *n_out = tot;
  return SA_OK;
}

int sa_expo_fast_probe(sa_engine *e, const uint64_t *d_ns, const int32_t *scale, uint64_t n, int32_t *fast,
                       int32_t *exact, double *log2_err) {
  if (!e || (n && (!d_ns || !scale || !fast || !exact)) || n > (1ULL << 20)) return SA_EINVAL;
  if (int rc = begin_read(e)) return rc;
  constexpr uint32_t kBlocks = 2048;
  char *buf = nullptr;
  if (int rc = dalloc(e, buf, n * 20 + kBlocks * 8, false, "probe buffer")) return rc;
  double *bmax = reinterpret_cast<double *>(buf);
  uint64_t *dd = reinterpret_cast<uint64_t *>(bmax + kBlocks);
  int32_t *ds = reinterpret_cast<int32_t *>(dd + n), *df = ds + n, *dx = df + n;
  hipError_t st = hipSuccess;
  if (n) {
    st = hipMemcpyAsync(dd, d_ns, n * 8, hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(ds, scale, n * 4, hipMemcpyHostToDevice, e->stream);
    if (st == hipSuccess) st = sa::launch_expo_fast_probe(dd, ds, n, unit_div(e), df, dx, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(fast, df, n * 4, hipMemcpyDeviceToHost, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(exact, dx, n * 4, hipMemcpyDeviceToHost, e->stream);
  }
  std::vector<double> hm(kBlocks);
  if (log2_err) {
    if (st == hipSuccess) st = sa::launch_log2_err_probe(0, 1u << 23, bmax, kBlocks, e->stream);
    if (st == hipSuccess) st = hipMemcpyAsync(hm.data(), bmax, kBlocks * 8, hipMemcpyDeviceToHost, e->stream);
  }
  if (st == hipSuccess) st = hipStreamSynchronize(e->stream);
  dfree(e, buf);
  if (st != hipSuccess) return fail(e, SA_EDEVICE, std::string("expo fast probe: ") + hipGetErrorString(st));
  if (log2_err) *log2_err = *std::max_element(hm.begin(), hm.end());
  return SA_OK;
}

int sa_window_read(sa_engine *e, uint64_t window_id, sa_sketch_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (!resident(e, window_id)) return fail(e, SA_ERANGE, "window not resident");
  if (int rc = begin_read(e)) return rc;
  const uint64_t ws = window_id & (e->cfg.n_windows - 1);
  if (int rc = fold_window(e, ws, e->stream)) return rc;
  auto *h = new sketch_holder();
  h->hll.resize(e->hll_slot_bytes);
  std::vector<uint64_t> cms64(e->cms_slot_elems);
  hipError_t a = hipMemcpyAsync(h->hll.data(), e->hll + ws * e->hll_slot_bytes, e->hll_slot_bytes,
                                hipMemcpyDeviceToHost, e->stream);
  hipError_t b = hipMemcpyAsync(cms64.data(), e->cms + ws * e->cms_slot_elems,
                                e->cms_slot_elems * 8, hipMemcpyDeviceToHost, e->stream);
  hipError_t c = hipStreamSynchronize(e->stream);
  if (a != hipSuccess || b != hipSuccess || c != hipSuccess) {
    delete h;
    return fail(e, SA_EDEVICE, "window read failed");
  }
  h->cms.resize(e->cms_slot_elems);
  for (size_t i = 0; i < cms64.size(); ++i)
    h->cms[i] = cms64[i] > UINT32_MAX ? UINT32_MAX : (uint32_t)cms64[i];
  h->wire(window_id, e->cfg);
  *out = &h->r;
  return SA_OK;
}

void sa_sketch_result_free(sa_sketch_result *r) { delete reinterpret_cast<sketch_holder *>(r); }

int sa_window_range(sa_engine *e, uint64_t first, uint64_t last, const uint64_t *keys, uint64_t n_keys, uint32_t flags,
                    sa_range_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = range_args(e, first, last, keys, n_keys, flags)) return rc;
  if (int rc = begin_read(e)) return rc;
  const bool regs = flags & SA_RANGE_REGISTERS, cells = n_keys || (flags & SA_RANGE_CELLS);
  if (int rc = range_buffers(e, n_keys, regs, cells)) return rc;
  const sa_engine::Range &R = e->range;
  // (without SA_RANGE_REGISTERS the merge writes the histogram and nothing else)
  if (int rc = range_merge_on(e, first, last, R.hist, regs ? R.regs : nullptr, cells ? R.cells : nullptr, e->stream))
    return rc;
  return range_result(e, first, last, R.hist, R.regs, R.cells, keys, n_keys, flags, e->stream, out);
}

void sa_range_result_free(sa_range_result *r) { delete reinterpret_cast<range_holder *>(r); }

int sa_window_series(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const uint64_t *keys,
                     uint64_t n_keys, uint32_t flags, sa_series_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (n_keys && !keys) return fail(e, SA_EINVAL, "window series: n_keys != 0 with null keys");
  if (flags) return fail(e, SA_EINVAL, "window series: flags are reserved (0)");
  const uint32_t W = e->cfg.n_windows;
  if (first > last || width == 0 || width > W || first + 1 < width || !resident(e, first - width + 1) ||
      !resident(e, last))
    return fail(e, SA_ERANGE, "window series: first > last, a width outside 1..n_windows, or a covered window is not resident");
  if (int rc = begin_read(e)) return rc;
  const uint64_t a = first - width + 1;
  const uint32_t n_out = (uint32_t)(last - first + 1), n_in = n_out + width - 1;  // (a and last resident: n_in <= W)
  std::unique_ptr<series_holder> h;
  std::vector<uint64_t> row0;
  try {
    h.reset(new series_holder());
    h->shape(first, last, width, e->cfg, n_keys);
    row0.resize(n_in);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window series: the result does not fit in host memory");
  }
  if (int rc = series_buffers(e, n_out, n_keys)) return rc;
  const sa_engine::Series &S = e->series;
  hipStream_t s = e->stream;
  // every covered window folded before any cell is read
  if (int rc = range_fold_on(e, a, last, s)) return rc;
  SA_HIP(e, sa::launch_series_hll(e->hll, W, e->cfg.n_services, e->cfg.hll_p, a, width, n_out, S.hist, s));
  SA_HIP(e, sa::launch_series_row0(e->cms, e->cms_slot_elems, W, a, n_in, e->cfg.cms_w, S.row0, s));
  hipError_t st = hipSuccess;
  if (n_keys) {
    st = hipMemcpyAsync(S.keys, keys, n_keys * 8, hipMemcpyHostToDevice, s);
    if (st == hipSuccess)
      st = sa::launch_series_query(e->cms, e->cms_slot_elems, W, a, width, n_out, e->cfg.cms_d, e->cfg.cms_w,
                                   64 - sa::log2u(e->cfg.cms_w), e->d_seeds, S.keys, n_keys, S.errors, s);
    if (st == hipSuccess) st = hipMemcpyAsync(h->errors.data(), S.errors, h->errors.size() * 8, hipMemcpyDeviceToHost, s);
  }
  if (st == hipSuccess) st = hipMemcpyAsync(h->hist.data(), S.hist, h->hist.size() * 4, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(row0.data(), S.row0, (size_t)n_in * 8, hipMemcpyDeviceToHost, s);
  const hipError_t waited = hipStreamSynchronize(s);  // (also after a failure: a copy into h may be in flight)
  if (st != hipSuccess || waited != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("window series: ") + hipGetErrorString(st != hipSuccess ? st : waited));
  uint64_t run = 0;  // the sliding sum of the windows' row-0 sums
  for (uint32_t k = 0; k < n_in; ++k) {
    run += row0[k];
    if (k >= width) run -= row0[k - width];
    if (k + 1 >= width) h->error_spans[k + 1 - width] = run;
  }
  for (size_t i = 0; i < h->distinct.size(); ++i)
    h->distinct[i] = sa_hll_estimate_hist(h->hist.data() + i * SA_HLL_HIST_BINS, e->cfg.hll_p);
  *out = &h.release()->r;
  return SA_OK;
}

void sa_series_result_free(sa_series_result *r) { delete reinterpret_cast<series_holder *>(r); }

int sa_window_top(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count, uint32_t flags,
                  sa_top_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (k == 0 || k > SA_TOP_MAX_K) return fail(e, SA_EINVAL, "window top: k outside 1..SA_TOP_MAX_K");
  if (flags) return fail(e, SA_EINVAL, "window top: flags are reserved (0)");
  if (int rc = range_args(e, first, last, nullptr, 0, 0)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = range_buffers(e, 0, false, true)) return rc;
  if (int rc = top_buffers(e)) return rc;
  unsigned long long *cells = e->range.cells;
  if (int rc = range_merge_on(e, first, last, nullptr, nullptr, cells, e->stream)) return rc;
  sa_grp::TopHost th;
  if (int rc = top_on(e, cells, k, min_count, e->stream, &th)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));  // the call's one wait
  if (int rc = sa_grp::top_result(first, last, k, &th, 1, out)) return fail(e, rc, "window top: the result does not fit in host memory");
  return SA_OK;
}

void sa_top_result_free(sa_top_result *r) { delete reinterpret_cast<top_holder *>(r); }

int sa_window_movers(sa_engine *e, uint64_t base_first, uint64_t base_last, uint64_t cur_first, uint64_t cur_last,
                     uint32_t k, uint64_t min_score, uint32_t flags, sa_movers_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (k == 0 || k > SA_TOP_MAX_K) return fail(e, SA_EINVAL, "window movers: k outside 1..SA_TOP_MAX_K");
  if (flags & ~SA_MOVERS_FALL) return fail(e, SA_EINVAL, "window movers: unknown flag bits");
  if (int rc = range_args(e, base_first, base_last, nullptr, 0, 0)) return rc;
  if (int rc = range_args(e, cur_first, cur_last, nullptr, 0, 0)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = range_buffers(e, 0, false, true)) return rc;
  sa_engine::Range &R = e->range;
  if (!R.cells_base)
    if (int rc = dalloc(e, R.cells_base, e->cms_slot_elems, false, "window movers: cell buffer hipMalloc failed")) return rc;
  if (int rc = movers_buffers(e)) return rc;
  if (int rc = range_merge_on(e, base_first, base_last, nullptr, nullptr, R.cells_base, e->stream)) return rc;
  if (int rc = range_merge_on(e, cur_first, cur_last, nullptr, nullptr, R.cells, e->stream)) return rc;
  sa_grp::MoversHost mh;
  if (int rc = movers_on(e, R.cells_base, R.cells, base_last - base_first + 1, cur_last - cur_first + 1, k, min_score,
                         flags, e->stream, &mh))
    return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));  // the call's one wait
  const uint64_t range[4] = {base_first, base_last, cur_first, cur_last};
  if (int rc = sa_grp::movers_result(range, k, flags, &mh, 1, out))
    return fail(e, rc, "window movers: the result does not fit in host memory");
  return SA_OK;
}

void sa_movers_result_free(sa_movers_result *r) { delete reinterpret_cast<movers_holder *>(r); }

int sa_window_overlap(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *services, uint32_t n_sel,
                      uint32_t flags, sa_overlap_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (flags) return fail(e, SA_EINVAL, "window overlap: flags are reserved (0)");
  std::vector<uint32_t> sel;
  try {
    if (const char *bad = sa_grp::overlap_select(e->cfg.n_services, services, n_sel, &sel)) return fail(e, SA_EINVAL, bad);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window overlap: the selection does not fit in host memory");
  }
  if (int rc = range_args(e, first, last, nullptr, 0, 0)) return rc;
  if (int rc = begin_read(e)) return rc;
  // (only the registers are read: no window's ERROR counts are folded)
  return overlap_on(e, first, last, e->hll, e->cfg.n_windows, first, (uint32_t)(last - first + 1), sel, e->stream, out);
}

void sa_overlap_result_free(sa_overlap_result *r) { delete reinterpret_cast<overlap_holder *>(r); }

int sa_window_latency(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const uint32_t *services,
                      uint32_t n_sel, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, sa_latency_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e)) return rc;
  std::vector<uint32_t> sel;
  try {
    if (const char *bad = sa_grp::latency_args(e->cfg.n_services, services, n_sel, q_ppm, n_q, flags, &sel))
      return fail(e, SA_EINVAL, bad);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency: the selection does not fit in host memory");
  }
  if (int rc = latency_range(e, first, last, width)) return rc;
  const uint32_t n_out = (uint32_t)(last - first + 1), S = (uint32_t)sel.size();
  if (const char *bad = sa_grp::latency_rows(n_out, S, flags)) return fail(e, SA_EINVAL, bad);
  if (int rc = begin_read(e)) return rc;
  std::unique_ptr<latency_holder> h = latency_result(e, first, last, width, sel, q_ppm, n_q, flags);
  if (!h) return SA_ENOMEM;
  // the outputs in tiles of at most kLatTileRows rows of sums (one tile's
  // sums, then its counts and bins, tile after tile on the engine stream)
  const uint32_t tile = (uint32_t)std::min<uint64_t>(n_out, std::max<uint64_t>(1, kLatTileRows / S));
  hipStream_t s = e->stream;
  if (int rc = latency_buffers(e, S, (uint64_t)tile * S, (uint64_t)n_out * S, n_q)) return rc;
  const sa_engine::Latency &L = e->lat;
  // (queued after everything that can fail without a wait: the copy reads the pageable `sel`
  // asynchronously, and latency_collect waits for `s`, whatever st says, before sel goes)
  hipError_t st = hipMemcpyAsync(L.sel, sel.data(), (size_t)S * 4, hipMemcpyHostToDevice, s);
  for (uint32_t o0 = 0; o0 < n_out && st == hipSuccess; o0 += tile) {
    const uint32_t n_o = std::min(tile, n_out - o0);
    st = sa::launch_lat_sums(L.ring, e->cfg.n_services, e->cfg.n_windows, L.sel, S, first - width + 1 + o0, width, n_o,
                             L.sums, s);
    if (st == hipSuccess) st = latency_scan_on(e, L.sums, (uint64_t)o0 * S, (uint64_t)n_o * S, h.get(), s);
  }
  return latency_collect(e, st, h, s, out);
}

void sa_latency_result_free(sa_latency_result *r) { delete reinterpret_cast<latency_holder *>(r); }

int sa_window_latency_movers(sa_engine *e, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                             uint64_t cur_last, uint32_t k, uint64_t min_count, uint32_t min_shift,
                             const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, sa_latency_movers_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e)) return rc;
  if (const char *bad = sa_grp::latency_movers_args(k, q_ppm, n_q, flags)) return fail(e, SA_EINVAL, bad);
  const uint64_t range[4] = {base_first, base_last, cur_first, cur_last};
  if (int rc = latency_movers_ranges(e, range)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = latency_movers_sums(e)) return rc;
  if (int rc = latency_movers_buffers(e)) return rc;
  // (the sums, then the stages a group runs on its member 0 after adding the members' sums)
  SA_HIP(e, latency_movers_sums_on(e, range, e->lat.mov_sums, e->stream));
  return sa_grp::window_latency_movers_finish(e, range, k, min_count, min_shift, q_ppm, n_q, flags,
                                              reinterpret_cast<const uint64_t *>(e->lat.mov_sums), e->stream, out);
}

void sa_latency_movers_result_free(sa_latency_movers_result *r) { delete reinterpret_cast<latency_movers_holder *>(r); }

int sa_window_advance(sa_engine *e, uint64_t new_base) {
  if (!e) return SA_EINVAL;
  if (new_base < e->win_base) return fail(e, SA_EINVAL, "window base cannot move backwards");
  if (new_base > UINT64_MAX / e->cfg.window_ns)
    return fail(e, SA_EINVAL, "window base beyond the u64 nanosecond range");
  if (int rc = begin_read(e)) return rc;
  const uint64_t n = std::min<uint64_t>(new_base - e->win_base, e->cfg.n_windows);
  for (uint64_t k = 0; k < n; ++k) {
    const uint64_t ws = (e->win_base + k) & (e->cfg.n_windows - 1);
    SA_HIP(e, hipMemsetAsync(e->hll + ws * e->hll_slot_bytes, 0, e->hll_slot_bytes, e->stream));
    if (e->hll_lb) {  // the window's bounds go back to 0 with its registers
      const size_t per = e->hll_slot_bytes >> e->lb_shift;
      SA_HIP(e, hipMemsetAsync(e->hll_lb + ws * per, 0, per, e->stream));
    }
    SA_HIP(e, hipMemsetAsync(e->cms + ws * e->cms_slot_elems, 0, e->cms_slot_elems * 8, e->stream));
    if (int rc = fold_errslab(e, ws, e->stream)) return rc;  // clears the slab cells
    SA_HIP(e, hipMemsetAsync(e->errcnt + ws * e->cap, 0, e->cap * 8, e->stream));
    if (e->lat.ring) {  // the window's latency histograms
      const size_t per = (size_t)e->cfg.n_services * SA_LAT_BINS;
      SA_HIP(e, hipMemsetAsync(e->lat.ring + ws * per, 0, per * 8, e->stream));
    }
  }
  e->win_base = new_base;
  return SA_OK;
}

int sa_debug_stamps(sa_engine *e, uint64_t *out, uint64_t cap, uint64_t *n_out) {
  if (!e || !n_out) return SA_EINVAL;
  *n_out = e->dbg ? (uint64_t)e->G * sa::kDbgPerWg : 0;
  if (!e->dbg || !out) return SA_OK;
  if (int rc = begin_read(e)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));
  SA_HIP(e, hipMemcpy(out, e->dbg, std::min<uint64_t>(cap, *n_out) * 8, hipMemcpyDeviceToHost));
  return SA_OK;
}

int sa_get_stats(sa_engine *e, sa_stats *o) {
  if (!e || !o) return SA_EINVAL;
  if (int rc = begin_read(e)) return rc;
  uint64_t st[sa::kNumStats];
  uint64_t nk = 0;
  if (int rc = count_keys(e, &nk)) return rc;
  if (int rc = read_stats(e, st)) return rc;
  if (e->dense()) nk = e->binned.n_bound;  // (the bound indices, as the host declared them)
  std::memset(o, 0, sizeof *o);
  o->spans = e->spans;
  o->zero_key = st[sa::kStatZeroKey];
  o->invalid_service = st[sa::kStatInvalidService];
  o->window_out_of_range = st[sa::kStatWindowOOR];
  o->dropped_table_full = st[sa::kStatDropped];
  o->n_keys = nk;
  o->table_capacity = e->cap;
  o->window_base = e->win_base;
  o->small_table = sa::lds_table(e->path) ? 1 : 0;
  {
    std::vector<uint64_t> f(sa::kFiltSlots);
    SA_HIP(e, hipMemcpyAsync(f.data(), e->hll_filt, sa::kFiltSlots * 8, hipMemcpyDeviceToHost, e->stream));
    SA_HIP(e, hipStreamSynchronize(e->stream));
    o->hll_filtered = std::accumulate(f.begin(), f.end(), (uint64_t)0);
  }
  return SA_OK;
}

int sa_bind_ids(sa_engine *e, const uint64_t *index, const uint64_t *key_hash, uint64_t n) {
  if (!e) return SA_EINVAL;
  if (!e->dense()) return fail(e, SA_ESTATE, "sa_bind_ids: the engine was not created with SA_OPT_DENSE_IDS");
  if (n == 0) return SA_OK;
  if (!index || !key_hash) return fail(e, SA_EINVAL, "sa_bind_ids: null array");
  sa_engine::Binned &b = e->binned;
  auto is_bound = [&](uint64_t i) { return (b.bound[i >> 6] >> (i & 63)) & 1u; };
  bool recycle = false;
  for (uint64_t j = 0; j < n; ++j) {
    if (index[j] == 0 || index[j] >= e->cap) return fail(e, SA_EINVAL, "sa_bind_ids: index 0 or at or past table_capacity");
    if (key_hash[j] == 0) return fail(e, SA_EINVAL, "sa_bind_ids: key_hash 0");
    recycle = recycle || is_bound(index[j]);
  }
  if (int rc = set_dev(e)) return rc;
  if (recycle) {
    // an index changes its series: only between a flush and the next ingest
    // (its row is zero then), and after every resident window's per-slot
    // ERROR counts went to the count-min under the old hash (as reclaim_now)
    if (e->unflushed) return fail(e, SA_ESTATE, "sa_bind_ids: rebinding an index with spans ingested since the last flush");
    if (int rc = join_checked(e)) return rc;
    if (int rc = fold_windows(e)) return rc;
  }
  if (b.bind_cap < n) {  // (hipFree waits for the device)
    dfree(e, b.bind_buf);
    b.bind_cap = 0;
    const uint64_t want = std::max<uint64_t>(n, 1u << 16);
    if (int rc = dalloc(e, b.bind_buf, want * 2, false, "sa_bind_ids: staging hipMalloc failed")) return rc;
    b.bind_cap = want;
  }
  // on the engine stream: after the previous bind's kernel (the staging's last
  // reader) and, through ev_ctl, before every later ingest on any stream.
  // Earlier launches still in flight do not read the key array.
  SA_HIP(e, hipMemcpyAsync(b.bind_buf, index, n * 8, hipMemcpyHostToDevice, e->stream));
  SA_HIP(e, hipMemcpyAsync(b.bind_buf + b.bind_cap, key_hash, n * 8, hipMemcpyHostToDevice, e->stream));
  SA_HIP(e, sa::launch_dn_bind(e->gkeys, b.bind_buf, b.bind_buf + b.bind_cap, n, b.log2sb, e->stream));
  // (the arrays are the caller's again when the call returns)
  SA_HIP(e, hipStreamSynchronize(e->stream));
  e->order.ctl_dirty = true;
  for (uint64_t j = 0; j < n; ++j)
    if (!is_bound(index[j])) {
      b.bound[index[j] >> 6] |= 1ULL << (index[j] & 63);
      ++b.n_bound;
    }
  return SA_OK;
}

int sa_export_keys(sa_engine *e, uint64_t *d_keys, uint64_t cap, uint64_t *n_out, void *stream) {
  if (!e || !n_out || (cap && !d_keys)) return SA_EINVAL;
  if (sa::expo_like(e->path)) return fail(e, SA_ESTATE, "merge hooks cover explicit-bucket engines only");
  if (int rc = begin_read(e)) return rc;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = export_keys_on(e, d_keys, cap, s)) return rc;
  SA_HIP(e, hipMemcpyAsync(n_out, e->scratch, 8, hipMemcpyDeviceToHost, s));
  SA_HIP(e, hipStreamSynchronize(s));
  return SA_OK;
}

int sa_gather_dense(sa_engine *e, const uint64_t *d_keys, uint64_t n, uint64_t *d_rows, int reset,
                    void *stream) {
  if (!e || (n && (!d_keys || !d_rows))) return SA_EINVAL;
  if (sa::expo_like(e->path)) return fail(e, SA_ESTATE, "merge hooks cover explicit-bucket engines only");
  if (e->dense()) return fail(e, SA_ESTATE, "sa_gather_dense: a dense-index engine has no hash -> slot map on the device");
  if (int rc = begin_read(e)) return rc;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = reduce_slabs(e, s)) return rc;
  SA_HIP(e, sa::launch_gather_dense(e->gkeys, e->gcounts, geom(e), d_keys, n, d_rows, s));
  if (reset) {
    e->unflushed = false;
    SA_HIP(e, hipMemsetAsync(e->gcounts, 0, counts_bytes(e), s));
    if (e->binned.base64)
      SA_HIP(e, hipMemsetAsync(e->binned.base64, 0, (size_t)e->cap * (e->hist.nbk + 1) * 8, s));
  }
  return hop_back(e, s);
}

int sa_window_export(sa_engine *e, uint64_t window_id, uint8_t *d_hll, uint64_t *d_cms,
                     void *stream) {
  if (!e) return SA_EINVAL;
  if (!resident(e, window_id)) return fail(e, SA_ERANGE, "window not resident");
  if (int rc = begin_read(e)) return rc;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  if (int rc = hop_to(e, s)) return rc;
  const uint64_t ws = window_id & (e->cfg.n_windows - 1);
  if (int rc = fold_window(e, ws, s)) return rc;
  if (d_hll)
    SA_HIP(e, hipMemcpyAsync(d_hll, e->hll + ws * e->hll_slot_bytes, e->hll_slot_bytes,
                             hipMemcpyDeviceToDevice, s));
  if (d_cms)
    SA_HIP(e, hipMemcpyAsync(d_cms, e->cms + ws * e->cms_slot_elems, e->cms_slot_elems * 8,
                             hipMemcpyDeviceToDevice, s));
  return hop_back(e, s);
}

}  // extern "C"
