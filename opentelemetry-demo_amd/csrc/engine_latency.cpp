// engine_latency.cpp -- the queries over the ring of latency histograms of an
// SA_OPT_WINDOW_LATENCY engine: sa_window_latency, sa_window_latency_movers,
// sa_window_slo and sa_window_latency_onset (kernels in spanagg_latency.hip, the
// movers' and the onset's select in spanagg_range.hip), each with the
// asynchronous halves the engine group runs per member (sa_grp,
// sa_group_hooks.h) and its result's free; and sa_onset_probe (spanagg_diag.h),
// the onset's scan on a caller's pairs.  Arguments: sa_query_args.h.  The
// queries share sa_engine::Latency's scratch, one buffer a role (sa_engine.h
// says why that is safe); the two ranked ones -- movers, onset -- share
// ranked_buffers and ranked_collect and differ in their launch and their rows.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "sa_engine.h"
#include "sa_group_hooks.h"
#include "sa_results.h"
#include "spanagg_diag.h"

namespace {

// ---- latency quantiles (sa_window_latency) ----
// rows of sliding sums one tile of outputs holds (64 MiB; at least one output's)
constexpr uint64_t kLatTileRows = 1u << 15;

// A stage's verdict (hipError_t or int: 0 is success), after a wait for `s` when
// it failed: a copy out of the caller's pageable arrays, or work in the engine's
// buffers, may be in flight.
template <class Rc>
Rc settled(Rc rc, hipStream_t s) {
  if (rc != 0) (void)hipStreamSynchronize(s);
  return rc;
}

int latency_enabled(sa_engine *e, const char *query) {
  if (const char *bad = sa_args::latency_option(e->cfg.options)) return bad_args(e, SA_ESTATE, query, bad);
  return SA_OK;
}

// Room for a selection of n_sel ids, sum_rows rows of sliding sums in the
// engine's own tile and `rows` rows' counts and quantile bins.
int latency_buffers(sa_engine *e, uint64_t n_sel, uint64_t sum_rows, uint64_t rows, uint32_t n_q) {
  sa_engine::Latency &L = e->lat;
  if (int rc = grow(e, L.sel, n_sel ? std::max<uint64_t>(n_sel, 64) : 0, "window latency: selection hipMalloc failed")) return rc;
  if (int rc = grow(e, L.sums, sum_rows * SA_LAT_BINS, "window latency: sum buffer hipMalloc failed")) return rc;
  if (int rc = grow(e, L.count, rows, "window latency: count buffer hipMalloc failed")) return rc;
  return grow(e, L.q_bin, rows * n_q, "window latency: quantile buffer hipMalloc failed");
}

// A member's part of a group query on `s`: the selection onto the device and
// the sums stage behind it, sums [n_out][sel.size()][SA_LAT_BINS] from window
// `a` on.  The copy reads the caller's pageable `sel` asynchronously, so it is
// queued after everything that can fail without a wait, and a failure behind
// it waits for `s` before it returns; on success the group waits before `sel` goes.
hipError_t latency_sums_on(sa_engine *e, const std::vector<uint32_t> &sel, uint64_t a, uint32_t width, uint32_t n_out,
                           unsigned long long *d_sums, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  hipError_t st = hipMemcpyAsync(L.sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s);
  if (st == hipSuccess)
    st = sa::launch_lat_sums(L.ring, e->cfg.n_services, e->cfg.n_windows, L.sel.p, (uint32_t)sel.size(), a, width, n_out,
                             d_sums, s);
  return settled(st, s);
}

// On `s`: the counts and quantile bins of rows row0 .. row0 + n_rows - 1 from
// their sums d_sums [n_rows][SA_LAT_BINS], and with SA_LAT_HIST the sums' copy
// into the result.
hipError_t latency_scan_on(sa_engine *e, const unsigned long long *d_sums, uint64_t row0, uint64_t n_rows,
                           latency_holder *h, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  const uint32_t n_q = h->r.n_q;
  hipError_t st = sa::launch_lat_scan(d_sums, n_rows, h->q_ppm.data(), n_q, L.count.p + row0, L.q_bin.p + row0 * n_q, s);
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
  if (st == hipSuccess) st = hipMemcpyAsync(h->count.data(), L.count.p, h->count.size() * 8, hipMemcpyDeviceToHost, s);
  if (st == hipSuccess) st = hipMemcpyAsync(h->q_bin.data(), L.q_bin.p, h->q_bin.size(), hipMemcpyDeviceToHost, s);
  if (int rc = wait_or_fail(e, st, s, "window latency")) return rc;
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

// ---- the two ranked queries' frame (latency movers, latency onset) ----
// What the stages after a ranked query's input work in: n_ids candidates (one
// an id), the ranked rows, and sa_window_top's control block.
int ranked_buffers(sa_engine *e, const std::string &query, uint64_t n_ids) {
  sa_engine::Latency &L = e->lat;
  if (int rc = lazy(e, e->top.ctl, 1, (query + ": control block hipMalloc failed").c_str())) return rc;
  if (int rc = lazy(e, L.ranked, 1, (query + ": row buffer hipMalloc failed").c_str())) return rc;
  return grow(e, L.cand, std::max<uint64_t>(n_ids, 64), (query + ": candidate buffer hipMalloc failed").c_str());
}

// What a ranked query brings back: TopCtl's head (the matches, the eligible
// ids, ..), the first k (score, id) pairs, the ranked block's head and first k
// rows, and n = the rows the answer has.
struct RankedHost {
  unsigned long long head[4] = {};
  std::vector<ulonglong2> sel;
  std::vector<unsigned long long> block;  // (its two head words, then the rows)
  uint32_t n = 0;
  template <class Row>
  Row row(uint32_t i) const {
    Row r;
    std::memcpy(&r, block.data() + 2 + (size_t)i * (sizeof r / 8), sizeof r);
    return r;
  }
};

// The stages after a ranked query's input on `s` -- launch(): the scan, the
// select and the sort, the selected rows of row_bytes each into e->lat.ranked
// -- the copies and the call's one wait.  ranked_buffers made room.
template <class Launch>
int ranked_collect(sa_engine *e, const char *query, uint32_t k, size_t row_bytes, hipStream_t s, RankedHost *h,
                   Launch launch) {
  try {
    h->sel.resize(k);
    h->block.resize(2 + (size_t)k * row_bytes / 8);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, std::string(query) + ": the rows do not fit in host memory");
  }
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  const hipError_t st =
      copy_ranked(launch(), e->top.ctl, k, h->head, h->sel.data(), e->lat.ranked, row_bytes, h->block.data(), s);
  if (int rc = wait_or_fail(e, st, s, query)) return rc;
  h->n = (uint32_t)std::min<uint64_t>(k, h->head[0]);
  return SA_OK;
}

// ---- latency movers (sa_window_latency_movers) ----
const char *const kLatMovers = "window latency movers";

// range: base first, base last, current first, current last
int latency_movers_ranges(sa_engine *e, const uint64_t range[4]) {
  if (int rc = check_span(e, kLatMovers, range[0], range[1], 1)) return rc;
  return check_span(e, kLatMovers, range[2], range[3], 1);
}

int latency_movers_buffers(sa_engine *e) {
  if (int rc = ranked_buffers(e, kLatMovers, e->cfg.n_services)) return rc;
  return lazy(e, e->lat.counts, 2 * (size_t)e->cfg.n_services, "window latency movers: count buffer hipMalloc failed");
}

// ---- latency SLO burn (sa_window_slo) ----
uint32_t slo_max_width(const uint32_t *widths, uint32_t n_widths) { return *std::max_element(widths, widths + n_widths); }

int slo_spans(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, uint32_t n_widths) {
  if (const char *bad = sa_args::slo_span(first, last, widths, n_widths, e->win_base, e->cfg.n_windows))
    return bad_args(e, SA_ERANGE, "window slo", bad);
  return SA_OK;
}

// Room for a selection of n_sel ids with their threshold bins.
int slo_selection(sa_engine *e, uint64_t n_sel) {
  sa_engine::Latency &L = e->lat;
  const uint64_t want = std::max<uint64_t>(n_sel, 64);
  if (int rc = grow(e, L.sel, want, "window slo: selection hipMalloc failed")) return rc;
  return grow(e, L.thr, want, "window slo: threshold buffer hipMalloc failed");
}

// A member's part of a query on `s`: the selection and its threshold bins onto
// the device and the pairs stage behind them, d_pairs [sel.size()][n_cov][2]
// from window `a` on.  The copies read the caller's pageable `sel` and `bins`
// asynchronously: as latency_sums_on's.
hipError_t slo_pairs_on(sa_engine *e, const std::vector<uint32_t> &sel, const std::vector<uint8_t> &bins, uint64_t a,
                        uint32_t n_cov, unsigned long long *d_pairs, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  hipError_t st = hipMemcpyAsync(L.sel.p, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, s);
  if (st == hipSuccess) st = hipMemcpyAsync(L.thr.p, bins.data(), bins.size(), hipMemcpyHostToDevice, s);
  if (st == hipSuccess)
    st = sa::launch_slo_pairs(L.ring, e->cfg.n_services, e->cfg.n_windows, L.sel.p, L.thr.p, (uint32_t)sel.size(), a,
                              n_cov, d_pairs, s);
  return settled(st, s);
}

// ---- latency onset (sa_window_latency_onset) ----
const char *const kOnset = "window latency onset";

// Room for n_sel ids' threshold bins and best splits, and for the ranked frame.
int onset_buffers(sa_engine *e, uint64_t n_sel) {
  sa_engine::Latency &L = e->lat;
  const uint64_t want = std::max<uint64_t>(n_sel, 64);
  if (int rc = ranked_buffers(e, kOnset, want)) return rc;
  if (int rc = grow(e, L.thr, want, "window latency onset: threshold buffer hipMalloc failed")) return rc;
  return grow(e, L.rec, want, "window latency onset: split buffer hipMalloc failed");
}

// A member's pairs stage on `s`: its threshold bins -- `bins` (host, one a
// service) copied, or the bins of quantile q_ppm of d_sums -- then d_pairs
// [n_services][n_cov][2] from window `first` on, every service selected.  The
// copy reads the caller's pageable `bins` asynchronously: as latency_sums_on's.
hipError_t onset_pairs_on(sa_engine *e, const uint8_t *bins, const unsigned long long *d_sums, uint32_t q_ppm,
                          uint64_t first, uint32_t n_cov, unsigned long long *d_pairs, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  const uint32_t S = e->cfg.n_services;
  hipError_t st = bins ? hipMemcpyAsync(L.thr.p, bins, S, hipMemcpyHostToDevice, s)
                       : sa::launch_onset_thr(d_sums, S, q_ppm, L.thr.p, s);
  if (st == hipSuccess) st = sa::launch_slo_pairs(L.ring, S, e->cfg.n_windows, nullptr, L.thr.p, S, first, n_cov, d_pairs, s);
  return settled(st, s);
}

// The stages after the pairs on `s` and the result: d_pairs [n_sel][n_cov][2]
// with n_cov = last - first + 1, d_thr [n_sel] the services' threshold bins
// (nullptr: the probe's, 0).  onset_buffers(e, n_sel) made room.
int onset_collect(sa_engine *e, uint64_t first, uint64_t last, uint32_t n_sel, uint32_t k, uint32_t q_ppm,
                  const uint8_t *d_thr, uint64_t min_count, uint32_t min_delta_ppm, uint32_t flags,
                  const unsigned long long *d_pairs, hipStream_t s, sa_onset_result **out) {
  const sa_engine::Latency &L = e->lat;
  const uint64_t mc = std::max<uint64_t>(min_count, 1);
  RankedHost rh;
  if (int rc = ranked_collect(e, kOnset, k, sizeof(sa::OnsetRow), s, &rh, [&] {
        return sa::launch_onset(d_pairs, n_sel, (uint32_t)(last - first + 1), k, mc, std::max(min_delta_ppm, 1u),
                                flags & SA_ONSET_FALL ? 1u : 0u, d_thr, L.rec.p, L.cand.p, e->top.ctl, &L.ranked->onset, s);
      }))
    return rc;
  std::unique_ptr<onset_holder> h;
  try {
    h.reset(new onset_holder());
    h->shape(first, last, k, rh.n, flags, q_ppm, mc, n_sel);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency onset: the result does not fit in host memory");
  }
  // (OnsetOut's head: the range's spans)
  h->r.n_matched = rh.head[0], h->r.n_eligible = rh.head[1], h->r.spans = rh.block[0];
  for (uint32_t i = 0; i < rh.n; ++i) {
    const sa::OnsetRow row = rh.row<sa::OnsetRow>(i);
    h->services[i] = (uint32_t)rh.sel[i].y;
    h->delta_ppm[i] = (int32_t)(rh.sel[i].x >> 44);
    h->onset_window[i] = first + row.t;
    h->total_before[i] = row.total_before, h->slow_before[i] = row.slow_before;
    h->total_after[i] = row.total_after, h->slow_after[i] = row.slow_after;
    h->threshold_bin[i] = (uint8_t)row.thr_bin;
    uint64_t lo = 0, hi = 0;
    if (d_thr) (void)sa_latency_bin_bounds((uint32_t)row.thr_bin, &lo, &hi);
    h->effective_ns[i] = hi;
  }
  *out = &h.release()->r;
  return SA_OK;
}
}  // namespace

namespace sa_grp {
int window_latency_export_async(sa_engine *e, uint64_t first, uint64_t last, uint32_t width,
                                const std::vector<uint32_t> &sel, uint64_t *d_sums, hipStream_t s) {
  if (!e || !d_sums || sel.empty()) return SA_EINVAL;
  if (int rc = latency_enabled(e, "window latency")) return rc;
  if (int rc = check_span(e, "window latency", first, last, width)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = latency_buffers(e, sel.size(), 0, 0, 0)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, latency_sums_on(e, sel, first - width + 1, width, (uint32_t)(last - first + 1),
                            reinterpret_cast<unsigned long long *>(d_sums), s));
  return settled(hop_back(e, s), s);  // (the selection buffer is the engine's)
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

int window_latency_movers_export_async(sa_engine *e, const uint64_t range[4], uint64_t *d_sums, hipStream_t s) {
  if (!e || !d_sums) return SA_EINVAL;
  if (int rc = latency_enabled(e, "window latency movers")) return rc;
  if (int rc = latency_movers_ranges(e, range)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, sa::launch_lat_range_sums(e->lat.ring, e->cfg.n_services, e->cfg.n_windows, range, 2,
                                      reinterpret_cast<unsigned long long *>(d_sums), s));
  return hop_back(e, s);  // (a later launch that writes the ring orders after these reads)
}

int window_latency_movers_finish(sa_engine *e, const uint64_t range[4], uint32_t k, uint64_t min_count,
                                 uint32_t min_shift, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                                 const uint64_t *d_sums, hipStream_t s, sa_latency_movers_result **out) {
  if (!e || !out || !d_sums) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = latency_movers_buffers(e)) return rc;
  const sa_engine::Latency &L = e->lat;
  RankedHost rh;
  if (int rc = ranked_collect(e, kLatMovers, k, sizeof(sa::LatMovRow), s, &rh, [&] {
        return sa::launch_lat_movers(reinterpret_cast<const unsigned long long *>(d_sums), e->cfg.n_services, k,
                                     std::max<uint64_t>(min_count, 1), std::max(min_shift, 1u),
                                     flags & SA_LATMOV_FALL ? 1u : 0u, q_ppm, n_q, L.counts, L.cand.p, e->top.ctl,
                                     &L.ranked->mov, s);
      }))
    return rc;
  std::unique_ptr<latency_movers_holder> h;
  try {
    h.reset(new latency_movers_holder());
    h->shape(range, k, rh.n, q_ppm, n_q, flags, e->cfg.n_services);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency movers: the result does not fit in host memory");
  }
  // (LatMovOut's head: the two ranges' spans)
  h->r.n_matched = rh.head[0], h->r.n_eligible = rh.head[1];
  h->r.spans_base = rh.block[0], h->r.spans_cur = rh.block[1];
  for (uint32_t i = 0; i < rh.n; ++i) {
    const sa::LatMovRow row = rh.row<sa::LatMovRow>(i);
    h->services[i] = (uint32_t)rh.sel[i].y;
    h->shift[i] = (int32_t)(rh.sel[i].x >> 48);
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

int window_slo_export_async(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, uint32_t n_widths,
                            const std::vector<uint32_t> &sel, const std::vector<uint8_t> &bins, uint64_t *d_pairs,
                            hipStream_t s) {
  if (!e || !d_pairs || !widths || !n_widths || sel.empty() || bins.size() != sel.size()) return SA_EINVAL;
  if (int rc = latency_enabled(e, "window slo")) return rc;
  if (int rc = slo_spans(e, first, last, widths, n_widths)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = slo_selection(e, sel.size())) return rc;
  if (int rc = hop_to(e, s)) return rc;
  const uint32_t mw = slo_max_width(widths, n_widths);
  SA_HIP(e, slo_pairs_on(e, sel, bins, first - mw + 1, (uint32_t)(last - first) + mw,
                         reinterpret_cast<unsigned long long *>(d_pairs), s));
  return settled(hop_back(e, s), s);  // (the selection buffers are the engine's)
}

int window_slo_finish(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, const uint32_t *limit_ppm,
                      uint32_t n_widths, const std::vector<uint32_t> &sel, const uint64_t *threshold_ns,
                      uint64_t min_count, const uint64_t *d_pairs, hipStream_t s, sa_slo_result **out) {
  if (!e || !out || !d_pairs || !widths || !limit_ppm || !n_widths || !threshold_ns || sel.empty()) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  const uint64_t mc = std::max<uint64_t>(min_count, 1);
  std::unique_ptr<slo_holder> h;
  try {
    std::vector<uint8_t> bins(sel.size());
    for (size_t i = 0; i < sel.size(); ++i) bins[i] = (uint8_t)sa_latency_bin(threshold_ns[i]);
    h.reset(new slo_holder());
    h->shape(first, last, widths, limit_ppm, n_widths, sel, threshold_ns, bins, mc);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window slo: the result does not fit in host memory");
  }
  for (size_t i = 0; i < sel.size(); ++i) {
    uint64_t lo = 0;
    (void)sa_latency_bin_bounds(h->threshold_bin[i], &lo, &h->effective_ns[i]);
  }
  // the answers in one buffer, laid out as the result's block (slo_holder): one copy brings them
  sa_engine::Latency &L = e->lat;
  const uint64_t S = sel.size(), n_out = h->r.n_out, n_cov = n_out + slo_max_width(widths, n_widths) - 1;
  if (int rc = grow(e, L.prefix, S * (n_cov + 1) * 2, "window slo: prefix buffer hipMalloc failed")) return rc;
  if (int rc = grow(e, L.slo_out, h->answers.size(), "window slo: answer buffer hipMalloc failed")) return rc;
  unsigned long long *d_total = L.slo_out.p, *d_slow = d_total + h->cells;
  uint32_t *d_alert = reinterpret_cast<uint32_t *>(d_slow + h->cells);
  uint8_t *d_burn = reinterpret_cast<uint8_t *>(d_slow + h->cells + h->alert_words);
  // (the scratch is the engine's: after its own earlier use, before its next)
  if (int rc = hop_to(e, s)) return rc;
  hipError_t st = sa::launch_slo_slide(reinterpret_cast<const unsigned long long *>(d_pairs), (uint32_t)S, (uint32_t)n_out,
                                       widths, limit_ppm, n_widths, mc, L.prefix.p, d_total, d_slow, d_burn, d_alert, s);
  if (st == hipSuccess)
    st = hipMemcpyAsync(h->answers.data(), L.slo_out.p, h->answers.size() * 8, hipMemcpyDeviceToHost, s);
  if (int rc = wait_or_fail(e, st, s, "window slo")) return rc;
  *out = &h.release()->r;
  return SA_OK;
}

int window_onset_sums_export_async(sa_engine *e, uint64_t first, uint64_t last, uint64_t *d_sums, hipStream_t s) {
  if (!e || !d_sums) return SA_EINVAL;
  if (int rc = latency_enabled(e, kOnset)) return rc;
  if (int rc = check_span(e, kOnset, first, last, 1)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  const uint64_t range[2] = {first, last};
  SA_HIP(e, sa::launch_lat_range_sums(e->lat.ring, e->cfg.n_services, e->cfg.n_windows, range, 1,
                                      reinterpret_cast<unsigned long long *>(d_sums), s));
  return hop_back(e, s);  // (a later launch that writes the ring orders after these reads)
}

int window_onset_pairs_export_async(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *bins,
                                    const uint64_t *d_sums, uint32_t q_ppm, uint64_t *d_pairs, hipStream_t s) {
  if (!e || !d_pairs || (!bins && !d_sums)) return SA_EINVAL;
  if (int rc = latency_enabled(e, kOnset)) return rc;
  if (int rc = check_span(e, kOnset, first, last, 1)) return rc;
  if (int rc = begin_read(e)) return rc;
  if (int rc = onset_buffers(e, e->cfg.n_services)) return rc;
  if (int rc = hop_to(e, s)) return rc;
  SA_HIP(e, onset_pairs_on(e, bins, reinterpret_cast<const unsigned long long *>(d_sums), q_ppm, first,
                           (uint32_t)(last - first + 1), reinterpret_cast<unsigned long long *>(d_pairs), s));
  return settled(hop_back(e, s), s);  // (the threshold buffer is the engine's)
}

int window_onset_finish(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint32_t q_ppm, bool pooled,
                        uint64_t min_count, uint32_t min_delta_ppm, uint32_t flags, const uint64_t *d_pairs,
                        hipStream_t s, sa_onset_result **out) {
  if (!e || !out || !d_pairs || first > last) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = onset_buffers(e, e->cfg.n_services)) return rc;  // (the pairs stage made them: nothing grows)
  return onset_collect(e, first, last, e->cfg.n_services, k, pooled ? q_ppm : 0, e->lat.thr.p, min_count,
                       min_delta_ppm, flags, reinterpret_cast<const unsigned long long *>(d_pairs), s, out);
}
}  // namespace sa_grp

extern "C" {

int sa_window_latency(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const uint32_t *services,
                      uint32_t n_sel, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, sa_latency_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e, "window latency")) return rc;
  std::vector<uint32_t> sel;
  try {
    if (const char *bad = sa_args::latency_args(e->cfg.n_services, services, n_sel, q_ppm, n_q, flags, &sel))
      return bad_args(e, SA_EINVAL, "window latency", bad);
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window latency: the selection does not fit in host memory");
  }
  if (int rc = check_span(e, "window latency", first, last, width)) return rc;
  const uint32_t n_out = (uint32_t)(last - first + 1), S = (uint32_t)sel.size();
  if (const char *bad = sa_args::latency_rows(n_out, S, flags)) return bad_args(e, SA_EINVAL, "window latency", bad);
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
  hipError_t st = hipMemcpyAsync(L.sel.p, sel.data(), (size_t)S * 4, hipMemcpyHostToDevice, s);
  for (uint32_t o0 = 0; o0 < n_out && st == hipSuccess; o0 += tile) {
    const uint32_t n_o = std::min(tile, n_out - o0);
    st = sa::launch_lat_sums(L.ring, e->cfg.n_services, e->cfg.n_windows, L.sel.p, S, first - width + 1 + o0, width, n_o,
                             L.sums.p, s);
    if (st == hipSuccess) st = latency_scan_on(e, L.sums.p, (uint64_t)o0 * S, (uint64_t)n_o * S, h.get(), s);
  }
  return latency_collect(e, st, h, s, out);
}

void sa_latency_result_free(sa_latency_result *r) { delete reinterpret_cast<latency_holder *>(r); }

int sa_window_latency_movers(sa_engine *e, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                             uint64_t cur_last, uint32_t k, uint64_t min_count, uint32_t min_shift,
                             const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, sa_latency_movers_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e, "window latency movers")) return rc;
  if (const char *bad = sa_args::latency_movers_args(k, q_ppm, n_q, flags))
    return bad_args(e, SA_EINVAL, "window latency movers", bad);
  const uint64_t range[4] = {base_first, base_last, cur_first, cur_last};
  if (int rc = latency_movers_ranges(e, range)) return rc;
  if (int rc = begin_read(e)) return rc;
  // both ranges' sums of the engine's own ring [2][n_services][SA_LAT_BINS]
  if (int rc = lazy(e, e->lat.range_sums, 2 * (size_t)e->cfg.n_services * SA_LAT_BINS,
                    "window latency movers: sum buffer hipMalloc failed"))
    return rc;
  if (int rc = latency_movers_buffers(e)) return rc;
  // (the sums, then the stages a group runs on its member 0 after adding the members' sums)
  SA_HIP(e, sa::launch_lat_range_sums(e->lat.ring, e->cfg.n_services, e->cfg.n_windows, range, 2, e->lat.range_sums, e->stream));
  return sa_grp::window_latency_movers_finish(e, range, k, min_count, min_shift, q_ppm, n_q, flags,
                                              reinterpret_cast<const uint64_t *>(e->lat.range_sums), e->stream, out);
}

void sa_latency_movers_result_free(sa_latency_movers_result *r) { delete reinterpret_cast<latency_movers_holder *>(r); }

int sa_window_slo(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, const uint32_t *limit_ppm,
                  uint32_t n_widths, const uint32_t *services, uint32_t n_sel, const uint64_t *threshold_ns,
                  uint64_t min_count, uint32_t flags, sa_slo_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e, "window slo")) return rc;
  std::vector<uint32_t> sel;
  std::vector<uint8_t> bins;
  try {
    if (const char *bad = sa_args::slo_args(e->cfg.n_services, widths, limit_ppm, n_widths, services, n_sel,
                                            threshold_ns, flags, &sel))
      return bad_args(e, SA_EINVAL, "window slo", bad);
    bins.resize(sel.size());
  } catch (const std::bad_alloc &) {
    return fail(e, SA_ENOMEM, "window slo: the selection does not fit in host memory");
  }
  for (size_t i = 0; i < sel.size(); ++i) bins[i] = (uint8_t)sa_latency_bin(threshold_ns[i]);
  if (int rc = slo_spans(e, first, last, widths, n_widths)) return rc;
  const uint32_t n_out = (uint32_t)(last - first + 1), S = (uint32_t)sel.size(), mw = slo_max_width(widths, n_widths);
  if (const char *bad = sa_args::slo_rows(n_out, S)) return bad_args(e, SA_EINVAL, "window slo", bad);
  if (int rc = begin_read(e)) return rc;
  const uint32_t n_cov = n_out + mw - 1;
  if (int rc = slo_selection(e, S)) return rc;
  if (int rc = grow(e, e->lat.pairs, (uint64_t)S * n_cov * 2, "window slo: pair buffer hipMalloc failed")) return rc;
  // (the pairs of the engine's own ring, then the stage a group runs on its member 0 after adding the
  // members' pairs; a failed launch has waited for the copies out of sel and bins)
  SA_HIP(e, slo_pairs_on(e, sel, bins, first - mw + 1, n_cov, e->lat.pairs.p, e->stream));
  // (a finish that failed early: the copies may be in flight)
  return settled(sa_grp::window_slo_finish(e, first, last, widths, limit_ppm, n_widths, sel, threshold_ns, min_count,
                                           reinterpret_cast<const uint64_t *>(e->lat.pairs.p), e->stream, out),
                 e->stream);
}

void sa_slo_result_free(sa_slo_result *r) { delete reinterpret_cast<slo_holder *>(r); }

int sa_window_latency_onset(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint32_t q_ppm,
                            const uint64_t *threshold_ns, uint64_t min_count, uint32_t min_delta_ppm, uint32_t flags,
                            sa_onset_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (int rc = latency_enabled(e, kOnset)) return rc;
  if (const char *bad = sa_args::onset_args(k, q_ppm, threshold_ns, flags)) return bad_args(e, SA_EINVAL, kOnset, bad);
  if (int rc = check_span(e, kOnset, first, last, 1)) return rc;
  const uint32_t S = e->cfg.n_services, n_cov = (uint32_t)(last - first + 1);
  std::vector<uint8_t> bins;
  if (threshold_ns) {
    try {
      bins.resize(S);
    } catch (const std::bad_alloc &) {
      return fail(e, SA_ENOMEM, "window latency onset: the thresholds do not fit in host memory");
    }
    for (uint32_t i = 0; i < S; ++i) bins[i] = (uint8_t)sa_latency_bin(threshold_ns[i]);
  }
  if (int rc = begin_read(e)) return rc;
  sa_engine::Latency &L = e->lat;
  if (int rc = onset_buffers(e, S)) return rc;
  if (int rc = grow(e, L.pairs, (uint64_t)S * n_cov * 2, "window latency onset: pair buffer hipMalloc failed")) return rc;
  if (!threshold_ns) {  // the pooled threshold: the range's rows of the engine's own ring summed
    if (int rc = lazy(e, L.range_sums, 2 * (size_t)S * SA_LAT_BINS, "window latency onset: sum buffer hipMalloc failed"))
      return rc;
    const uint64_t range[2] = {first, last};
    SA_HIP(e, sa::launch_lat_range_sums(L.ring, S, e->cfg.n_windows, range, 1, L.range_sums, e->stream));
  }
  // (the pairs of the engine's own ring, then the stages a group runs on its member 0 after adding the
  // members' pairs; a failed launch has waited for the copy out of bins)
  SA_HIP(e, onset_pairs_on(e, threshold_ns ? bins.data() : nullptr, L.range_sums, q_ppm, first, n_cov, L.pairs.p,
                           e->stream));
  // (a collect that failed early: the copy may be in flight)
  return settled(onset_collect(e, first, last, S, k, q_ppm, L.thr.p, min_count, min_delta_ppm, flags, L.pairs.p, e->stream,
                               out),
                 e->stream);
}

void sa_onset_result_free(sa_onset_result *r) { delete reinterpret_cast<onset_holder *>(r); }

int sa_onset_probe(sa_engine *e, const uint64_t *pairs, uint32_t n_sel, uint32_t n_cov, uint32_t k, uint64_t min_count,
                   uint32_t min_delta_ppm, uint32_t flags, sa_onset_result **out) {
  if (!e || !out) return SA_EINVAL;
  *out = nullptr;
  if (!pairs || !n_sel || !n_cov || (uint64_t)n_sel * n_cov > (1ull << 18))
    return bad_args(e, SA_EINVAL, "onset probe", "null pairs, or n_sel * n_cov outside 1..2^18");
  if (const char *bad = sa_args::top_k(k)) return bad_args(e, SA_EINVAL, "onset probe", bad);
  if (const char *bad = sa_args::flags(flags, SA_ONSET_FALL)) return bad_args(e, SA_EINVAL, "onset probe", bad);
  if (int rc = begin_read(e)) return rc;
  sa_engine::Latency &L = e->lat;
  if (int rc = onset_buffers(e, n_sel)) return rc;
  if (int rc = grow(e, L.pairs, (uint64_t)n_sel * n_cov * 2, "onset probe: pair buffer hipMalloc failed")) return rc;
  // (the copy reads the caller's pageable pairs asynchronously: the collect waits for the stream)
  SA_HIP(e, hipMemcpyAsync(L.pairs.p, pairs, (size_t)n_sel * n_cov * 16, hipMemcpyHostToDevice, e->stream));
  return settled(onset_collect(e, 0, n_cov - 1, n_sel, k, 0, nullptr, min_count, min_delta_ppm, flags, L.pairs.p, e->stream,
                               out),
                 e->stream);
}

}  // extern "C"
