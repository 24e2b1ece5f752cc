// engine_window.cpp -- the queries over the ring of window sketches:
// sa_window_range, _series, _top, _movers, _error_onset and _overlap (kernels
// in spanagg_range.hip, spanagg_error_onset.hip and spanagg_overlap.hip), each with the asynchronous
// halves the engine group runs per member (sa_grp, sa_group_hooks.h) and its
// result's free.  Every query checks its arguments (sa_query_args.h), joins
// the launches in flight (begin_read), sizes its scratch, queues its work on
// one stream and waits once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <memory>
#include <new>
#include <string>
#include <tuple>
#include <vector>

#include "sa_engine.h"
#include "sa_group_hooks.h"
#include "sa_results.h"

// sa::TopCtl's head and its first k selected rows to the host, on `s`
static hipError_t copy_top(const sa::TopCtl *ctl, uint32_t k, unsigned long long head[4], ulonglong2 *rows, hipStream_t s) {
  const hipError_t st = hipMemcpyAsync(head, ctl, 4 * sizeof head[0], hipMemcpyDeviceToHost, s);
  return st != hipSuccess ? st : hipMemcpyAsync(rows, ctl->sel, (size_t)k * 16, hipMemcpyDeviceToHost, s);
}

static_assert(offsetof(sa::MoversOut, est) == 16 && offsetof(sa::LatMovOut, row) == 16 && offsetof(sa::OnsetOut, row) == 16 &&
                  offsetof(sa::ErrOnsetOut, row) == 16,
              "a ranked block's head");
hipError_t copy_ranked(hipError_t st, const sa::TopCtl *ctl, uint32_t k, unsigned long long head[4], ulonglong2 *sel,
                       const void *d_out, size_t row_bytes, void *block, hipStream_t s) {
  if (st == hipSuccess) st = copy_top(ctl, k, head, sel, s);
  if (st == hipSuccess) st = hipMemcpyAsync(block, d_out, 16 + (size_t)k * row_bytes, hipMemcpyDeviceToHost, s);
  return st;
}

namespace {

// ---- range queries (sa_window_range) ----
// the engine's own device buffers: the histogram, room for n_keys keys and
// their answers, and the merged registers / summed cells where asked for
int range_buffers(sa_engine *e, uint64_t n_keys, bool regs, bool cells) {
  sa_engine::Range &R = e->range;
  if (int rc = lazy(e, R.hist, (size_t)e->cfg.n_services * SA_HLL_HIST_BINS, "window range: histogram hipMalloc failed"))
    return rc;
  if (regs)
    if (int rc = lazy(e, R.regs, e->hll_slot_bytes, "window range: register buffer hipMalloc failed")) return rc;
  if (cells)
    if (int rc = lazy(e, R.cells, e->cms_slot_elems, "window range: cell buffer hipMalloc failed")) return rc;
  if (2 * n_keys <= R.keys.cap) return SA_OK;  // (the keys and their answers: the two halves of one allocation)
  return grow(e, R.keys, 2 * std::max<uint64_t>(n_keys, 1u << 10), "window range: key buffer hipMalloc failed");
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
    uint64_t *dk = e->range.keys.p, *de = dk + e->range.keys.cap / 2;
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
  if (int rc = wait_or_fail(e, st, s, "window range")) return rc;
  for (uint32_t sv = 0; sv < e->cfg.n_services; ++sv)
    h->distinct[sv] = sa_hll_estimate_hist(h->hist.data() + (size_t)sv * SA_HLL_HIST_BINS, e->cfg.hll_p);
  *out = &h.release()->r;
  return SA_OK;
}

// ---- sliding series (sa_window_series) ----
int series_buffers(sa_engine *e, uint64_t n_out, uint64_t n_keys) {
  sa_engine::Series &S = e->series;
  if (int rc = grow(e, S.hist, n_out * e->cfg.n_services * SA_HLL_HIST_BINS,
                    "window series: histogram hipMalloc failed"))
    return rc;
  if (int rc = lazy(e, S.row0, e->cfg.n_windows, "window series: row sum hipMalloc failed")) return rc;
  if (int rc = grow(e, S.keys, n_keys ? std::max<uint64_t>(n_keys, 1u << 10) : 0,
                    "window series: key buffer hipMalloc failed"))
    return rc;
  return grow(e, S.errors, n_out * n_keys, "window series: answer buffer hipMalloc failed");
}

// ---- heavy hitters (sa_window_top) ----
int top_buffers(sa_engine *e) {
  if (int rc = lazy(e, e->top.cand, e->cap, "window top: candidate buffer hipMalloc failed")) return rc;
  return lazy(e, e->top.ctl, 1, "window top: control block hipMalloc failed");
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
  if (st == hipSuccess) st = copy_top(T.ctl, k, h->head, h->rows.data(), s);
  return st == hipSuccess ? SA_OK : wait_or_fail(e, st, s, "window top");  // (a copy into h may be in flight)
}

// ---- movers (sa_window_movers) ----
int movers_buffers(sa_engine *e) {
  if (int rc = top_buffers(e)) return rc;  // (the candidates and the select's state: calls are serialised)
  return lazy(e, e->movers.out, 1, "window movers: estimate buffer hipMalloc failed");
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
  st = copy_ranked(st, T.ctl, k, h->top.head, h->top.rows.data(), O, sizeof O->est[0], h->out.data(), s);
  return st == hipSuccess ? SA_OK : wait_or_fail(e, st, s, "window movers");  // (a copy into h may be in flight)
}

// ---- error onset (sa_window_error_onset) ----
// The scan's lane mapping: the laboratory build reads SPANAGG_EO_WAVE (0, 1) at
// every call, the product holds variant 0 alone.
uint32_t error_onset_variant() {
#ifdef SPANAGG_AB
  if (const char *v = ab_env("SPANAGG_EO_WAVE")) return (uint32_t)std::atoi(v);
#endif
  return 0;
}

int error_onset_buffers(sa_engine *e) {
  if (int rc = top_buffers(e)) return rc;  // (the candidates and the select's state: calls are serialised)
  return lazy(e, e->err_onset.out, 1, "window error onset: split buffer hipMalloc failed");
}

// On `s`, not waited for: e's key table scanned against d_sum [d][w] -- the
// range's n windows summed -- and the windows themselves (window j at d_win +
// ((first + j) & mask) * the slot's cells), the first k matches selected and
// sorted, the counters, the k rows and their splits copied into *h.
int error_onset_on(sa_engine *e, const unsigned long long *d_sum, const unsigned long long *d_win, uint64_t first,
                   uint64_t mask, uint32_t n, uint32_t k, uint64_t min_count, uint64_t min_score, uint32_t flags,
                   hipStream_t s, sa_grp::ErrOnsetHost *h) {
  const sa_engine::Top &T = e->top;
  sa::ErrOnsetOut *O = e->err_onset.out;
  try {
    h->top.rows.resize(k);
    h->out.resize(2 + 3 * (size_t)k);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window error onset: the rows do not fit in host memory");
  }
  hipError_t st = sa::launch_error_onset(e->gkeys, e->cap, e->binned.kinv, d_sum, d_win, e->cms_slot_elems, first, mask, n,
                                         e->cfg.cms_d, e->cfg.cms_w, 64 - sa::log2u(e->cfg.cms_w), e->d_seeds,
                                         flags & SA_ERROR_ONSET_FALL ? 1u : 0u, k, std::max<uint64_t>(min_count, 1),
                                         std::max<uint64_t>(min_score, 1), T.cand, T.ctl, O, error_onset_variant(), s);
  st = copy_ranked(st, T.ctl, k, h->top.head, h->top.rows.data(), O, sizeof O->row[0], h->out.data(), s);
  return st == hipSuccess ? SA_OK : wait_or_fail(e, st, s, "window error onset");  // (a copy into h may be in flight)
}

// ---- service overlap (sa_window_overlap) ----
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
  if (int rc = lazy(e, O.map, cap, "window overlap: selection hipMalloc failed")) return rc;
  if (int rc = lazy(e, O.hist, cap * SA_HLL_HIST_BINS, "window overlap: histogram hipMalloc failed")) return rc;
  if (int rc = lazy(e, O.pair_hist, cap * (cap - 1) / 2 * SA_HLL_HIST_BINS, "window overlap: pair histogram hipMalloc failed"))
    return rc;
  return lazy(e, O.regs, cap << e->cfg.hll_p, "window overlap: register buffer hipMalloc failed");
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
  if (int rc = wait_or_fail(e, st, s, "window overlap")) return rc;
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
std::vector<Ranked> ranked_rows(uint32_t k, const sa_grp::TopHost *const *m, const ulonglong2 *const *extra, uint32_t n) {
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

namespace sa_grp {
int window_range_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, uint64_t *d_cms,
                              hipStream_t s) {
  if (!e || !d_cms) return SA_EINVAL;
  if (int rc = check_span(e, "window range", first, last)) return rc;
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

int window_cells_export_async(sa_engine *e, uint64_t first, uint64_t last, uint64_t *d_win, hipStream_t s) {
  if (!e || !d_win) return SA_EINVAL;
  if (int rc = check_span(e, "window error onset", first, last)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  if (int rc = range_fold_on(e, first, last, s)) return rc;
  // the ring wraps: the slots from first's to the ring's end, then the ring's start
  const uint64_t W = e->cfg.n_windows, n = last - first + 1, at = first & (W - 1), head = std::min(n, W - at);
  const size_t slot = e->cms_slot_elems;
  SA_HIP(e, hipMemcpyAsync(d_win, e->cms + at * slot, head * slot * 8, hipMemcpyDeviceToDevice, s));
  if (n > head) SA_HIP(e, hipMemcpyAsync(d_win + head * slot, e->cms, (n - head) * slot * 8, hipMemcpyDeviceToDevice, s));
  return hop_back(e, s);  // (the folds wrote this engine's cells and ERROR counts)
}

int window_error_onset_async(sa_engine *e, const uint64_t *d_win, uint32_t n, uint32_t k, uint64_t min_count,
                             uint64_t min_score, uint32_t flags, hipStream_t s, ErrOnsetHost *out) {
  if (!e || !d_win || !out || !n) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = range_buffers(e, 0, false, true)) return rc;
  if (int rc = error_onset_buffers(e)) return rc;
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  const unsigned long long *win = reinterpret_cast<const unsigned long long *>(d_win);
  uint32_t ring = 1;  // the unwrapped array as a ring that never wraps
  while (ring < n) ring <<= 1;
  SA_HIP(e, sa::launch_range_cells(win, e->cms_slot_elems, ring, 0, n, e->range.cells, s));
  if (int rc = error_onset_on(e, e->range.cells, win, 0, ~0ULL, n, k, min_count, min_score, flags, s, out)) return rc;
  return hop_back(e, s);
}

int error_onset_result(uint64_t first, uint64_t last, uint32_t k, uint32_t flags, const ErrOnsetHost *m,
                       uint32_t n_members, sa_error_onset_result **out) {
  try {
    std::unique_ptr<error_onset_holder> h(new error_onset_holder());
    // a row: key, D, t, B, A -- one member's as they are, the device's order; several members' merged as
    // ranked_rows merges (a series on several members has the same row on each: once)
    std::vector<std::array<uint64_t, 5>> all;
    for (uint32_t j = 0; j < n_members; ++j) {
      const size_t rows = (size_t)std::min<uint64_t>(k, m[j].top.head[0]);
      const unsigned long long *split = m[j].out.data() + 2;
      for (size_t i = 0; i < rows; ++i)
        all.push_back({m[j].top.rows[i].y, m[j].top.rows[i].x, split[3 * i], split[3 * i + 1], split[3 * i + 2]});
    }
    if (n_members > 1) {
      std::sort(all.begin(), all.end());
      all.erase(std::unique(all.begin(), all.end()), all.end());
      std::sort(all.begin(), all.end(), [](const std::array<uint64_t, 5> &a, const std::array<uint64_t, 5> &b) {
        return a[1] != b[1] ? a[1] > b[1] : a[0] < b[0];
      });
      if (all.size() > k) all.resize(k);
    }
    h->shape(first, last, k, (uint32_t)all.size(), flags);
    for (size_t i = 0; i < all.size(); ++i) {
      h->keys[i] = all[i][0], h->score[i] = (int64_t)all[i][1];  // (a match's score is >= 1)
      h->onset[i] = first + all[i][2], h->before[i] = all[i][3], h->after[i] = all[i][4];
    }
    for (uint32_t j = 0; j < n_members; ++j) {
      h->r.n_matched += m[j].top.head[0], h->r.n_resident += m[j].top.head[1];
      h->r.n_eligible += m[j].out[0];
    }
    h->r.error_spans = m[0].top.head[3];  // (the merged cells are the same on every member)
    *out = &h.release()->r;
    return SA_OK;
  } catch (const std::bad_alloc &) {
    return SA_ENOMEM;
  }
}

int window_overlap_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, hipStream_t s) {
  if (!e || !d_hll) return SA_EINVAL;
  if (int rc = check_span(e, "window overlap", first, last)) return rc;
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
}  // namespace sa_grp

extern "C" {

int sa_window_range(sa_engine *e, uint64_t first, uint64_t last, const uint64_t *keys, uint64_t n_keys, uint32_t flags,
                    sa_range_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (const char *bad = sa_args::keys(keys, n_keys)) return bad_args(e, SA_EINVAL, "window range", bad);
  if (const char *bad = sa_args::flags(flags, SA_RANGE_REGISTERS | SA_RANGE_CELLS))
    return bad_args(e, SA_EINVAL, "window range", bad);
  if (int rc = check_span(e, "window range", first, last)) return rc;
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
  if (const char *bad = sa_args::keys(keys, n_keys)) return bad_args(e, SA_EINVAL, "window series", bad);
  if (const char *bad = sa_args::flags(flags, 0)) return bad_args(e, SA_EINVAL, "window series", bad);
  if (int rc = check_span(e, "window series", first, last, width)) return rc;
  if (int rc = begin_read(e)) return rc;
  const uint32_t W = e->cfg.n_windows;
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
  SA_HIP(e, sa::launch_series_hll(e->hll, W, e->cfg.n_services, e->cfg.hll_p, a, width, n_out, S.hist.p, s));
  SA_HIP(e, sa::launch_series_row0(e->cms, e->cms_slot_elems, W, a, n_in, e->cfg.cms_w, S.row0, s));
  hipError_t st = hipSuccess;
  if (n_keys) {
    st = hipMemcpyAsync(S.keys.p, keys, n_keys * 8, hipMemcpyHostToDevice, s);
    if (st == hipSuccess)
      st = sa::launch_series_query(e->cms, e->cms_slot_elems, W, a, width, n_out, e->cfg.cms_d, e->cfg.cms_w,
                                   64 - sa::log2u(e->cfg.cms_w), e->d_seeds, S.keys.p, n_keys, S.errors.p, s);
    if (st == hipSuccess) st = hipMemcpyAsync(h->errors.data(), S.errors.p, h->errors.size() * 8, hipMemcpyDeviceToHost, s);
  }
  if (st == hipSuccess) st = hipMemcpyAsync(h->hist.data(), S.hist.p, h->hist.size() * 4, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(row0.data(), S.row0, (size_t)n_in * 8, hipMemcpyDeviceToHost, s);
  if (int rc = wait_or_fail(e, st, s, "window series")) return rc;
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
  if (const char *bad = sa_args::top_k(k)) return bad_args(e, SA_EINVAL, "window top", bad);
  if (const char *bad = sa_args::flags(flags, 0)) return bad_args(e, SA_EINVAL, "window top", bad);
  if (int rc = check_span(e, "window top", first, last)) return rc;
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
  if (const char *bad = sa_args::top_k(k)) return bad_args(e, SA_EINVAL, "window movers", bad);
  if (const char *bad = sa_args::flags(flags, SA_MOVERS_FALL)) return bad_args(e, SA_EINVAL, "window movers", bad);
  if (int rc = check_span(e, "window movers", base_first, base_last)) return rc;
  if (int rc = check_span(e, "window movers", cur_first, cur_last)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = range_buffers(e, 0, false, true)) return rc;
  sa_engine::Range &R = e->range;
  if (int rc = lazy(e, R.cells_base, e->cms_slot_elems, "window movers: cell buffer hipMalloc failed")) return rc;
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

int sa_window_error_onset(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count,
                          uint64_t min_score, uint32_t flags, sa_error_onset_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (const char *bad = sa_args::error_onset_args(k, flags)) return bad_args(e, SA_EINVAL, "window error onset", bad);
  if (int rc = check_span(e, "window error onset", first, last)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = range_buffers(e, 0, false, true)) return rc;
  if (int rc = error_onset_buffers(e)) return rc;
  unsigned long long *cells = e->range.cells;
  // every window of the range folded and summed, then the walk over the ring's own cells
  if (int rc = range_merge_on(e, first, last, nullptr, nullptr, cells, e->stream)) return rc;
  sa_grp::ErrOnsetHost eh;
  if (int rc = error_onset_on(e, cells, e->cms, first, e->cfg.n_windows - 1, (uint32_t)(last - first + 1), k, min_count,
                              min_score, flags, e->stream, &eh))
    return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));  // the call's one wait
  if (int rc = sa_grp::error_onset_result(first, last, k, flags, &eh, 1, out))
    return fail(e, rc, "window error onset: the result does not fit in host memory");
  return SA_OK;
}

void sa_error_onset_result_free(sa_error_onset_result *r) { delete reinterpret_cast<error_onset_holder *>(r); }

int sa_window_overlap(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *services, uint32_t n_sel,
                      uint32_t flags, sa_overlap_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (const char *bad = sa_args::flags(flags, 0)) return bad_args(e, SA_EINVAL, "window overlap", bad);
  std::vector<uint32_t> sel;
  try {
    if (const char *bad = sa_args::overlap_select(e->cfg.n_services, services, n_sel, &sel))
      return bad_args(e, SA_EINVAL, "window overlap", bad);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window overlap: the selection does not fit in host memory");
  }
  if (int rc = check_span(e, "window overlap", first, last)) return rc;
  if (int rc = begin_read(e)) return rc;
  // (only the registers are read: no window's ERROR counts are folded)
  return overlap_on(e, first, last, e->hll, e->cfg.n_windows, first, (uint32_t)(last - first + 1), sel, e->stream, out);
}

void sa_overlap_result_free(sa_overlap_result *r) { delete reinterpret_cast<overlap_holder *>(r); }

}  // extern "C"
