// sa_results.h -- host-side result holders shared by the engine and the group
// (sa_red_result_free / sa_sketch_result_free delete these).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "spanagg.h"

// Page-locked result blocks reused across flushes.  A flush at C4 scale hands
// back ~170 MB of columns; pageable std::vector columns cost a zero fill (and
// its page faults) plus a staged D2H copy, so a group flush DMAs into one of
// these blocks instead.  A result holds its block until sa_red_result_free,
// which returns it here; the pool is shared with the results, so a result
// may outlive the group that made it.
struct PinPool {
  std::mutex mu;
  std::vector<std::pair<void *, size_t>> blocks;  // free blocks
  static constexpr size_t kKeep = 2;              // free blocks kept for the next flushes
  ~PinPool() {
    for (auto &b : blocks) (void)hipHostFree(b.first);
  }
  // a free block of at least `bytes` (the smallest that fits), else a new one
  void *take(size_t bytes, size_t *got) {
    {
      std::lock_guard<std::mutex> l(mu);
      size_t best = blocks.size();
      for (size_t i = 0; i < blocks.size(); ++i)
        if (blocks[i].second >= bytes && (best == blocks.size() || blocks[i].second < blocks[best].second)) best = i;
      if (best < blocks.size()) {
        auto b = blocks[best];
        blocks.erase(blocks.begin() + (long)best);
        *got = b.second;
        return b.first;
      }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    *got = bytes;
    return p;
  }
  void give(void *p, size_t bytes) {
    void *drop = p;
    {
      std::lock_guard<std::mutex> l(mu);
      if (blocks.size() < kKeep) {
        blocks.emplace_back(p, bytes);
        drop = nullptr;
      } else {  // keep the larger blocks: a flush needs one at least as large as the last
        size_t small = 0;
        for (size_t i = 1; i < blocks.size(); ++i)
          if (blocks[i].second < blocks[small].second) small = i;
        if (blocks[small].second < bytes) {
          drop = blocks[small].first;
          blocks[small] = std::make_pair(p, bytes);
        }
      }
    }
    if (drop) (void)hipHostFree(drop);
  }
};

struct red_holder {
  sa_red_result r;
  std::vector<uint64_t> keys, counts, calls, sum_ns;
  std::vector<double> sum;
  // columns in a page-locked block of `pool` (group flush) instead of the vectors
  std::shared_ptr<PinPool> pool;
  void *pin = nullptr;
  size_t pin_bytes = 0;
  ~red_holder() {
    if (pin) pool->give(pin, pin_bytes);
  }
  // the vector columns sized for n series of nbk buckets, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t n, uint32_t nbk) {
    keys.resize(n), counts.resize(n * nbk), calls.resize(n), sum_ns.resize(n), sum.resize(n);
    r.n_series = n, r.n_buckets = nbk;
    r.key_hash = keys.data(), r.bucket_counts = counts.data(), r.calls = calls.data();
    r.sum_ns = sum_ns.data(), r.sum = sum.data();
  }
};

struct exp_holder {
  sa_exp_result r;
  std::vector<uint64_t> keys, count, zero, sum_ns, buckets;
  std::vector<double> sum, min, max;
  std::vector<int32_t> scale, offset;
  std::vector<uint32_t> nb;
  // the columns sized for n series of at most max_size buckets (zeroed), and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t n, uint32_t max_size, uint32_t unit) {
    keys.resize(n), count.resize(n), zero.resize(n), sum_ns.resize(n), sum.resize(n), min.resize(n), max.resize(n);
    scale.resize(n), offset.resize(n), nb.resize(n), buckets.assign(n * max_size, 0);
    r.n_series = n, r.max_size = max_size, r.unit = unit;
    r.key_hash = keys.data(), r.count = count.data(), r.zero_count = zero.data(), r.sum_ns = sum_ns.data();
    r.sum = sum.data(), r.min = min.data(), r.max = max.data(), r.scale = scale.data(), r.offset = offset.data();
    r.n_buckets = nb.data(), r.bucket_counts = buckets.data();
  }
};

struct range_holder {
  sa_range_result r;
  std::vector<uint32_t> hist;
  std::vector<double> distinct;
  std::vector<uint8_t> hll;
  std::vector<uint64_t> cms, errors;
  // the columns sized for config c, n_keys keys and the flags' optional parts, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, const sa_config &c, uint64_t n_keys,
                                                   uint32_t flags) {
    hist.resize((size_t)c.n_services * SA_HLL_HIST_BINS), distinct.resize(c.n_services), errors.resize(n_keys);
    if (flags & SA_RANGE_REGISTERS) hll.resize((size_t)c.n_services << c.hll_p);
    if (flags & SA_RANGE_CELLS) cms.resize((size_t)c.cms_d * c.cms_w);
    r.first_window = first, r.last_window = last, r.n_services = c.n_services, r.hll_p = c.hll_p;
    r.hll_hist = hist.data(), r.distinct = distinct.data();
    r.hll = (flags & SA_RANGE_REGISTERS) ? hll.data() : nullptr;
    r.cms_d = c.cms_d, r.cms_w = c.cms_w, r.cms = (flags & SA_RANGE_CELLS) ? cms.data() : nullptr;
    r.n_keys = n_keys, r.errors = errors.data();
  }
};

struct series_holder {
  sa_series_result r;
  std::vector<uint32_t> hist;
  std::vector<double> distinct;
  std::vector<uint64_t> error_spans, errors;
  // the columns sized for outputs first..last of config c and n_keys keys, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, uint32_t width, const sa_config &c,
                                                   uint64_t n_keys) {
    const size_t n_out = (size_t)(last - first + 1);
    hist.resize(n_out * c.n_services * SA_HLL_HIST_BINS), distinct.resize(n_out * c.n_services);
    error_spans.resize(n_out), errors.resize(n_out * n_keys);
    r.first_window = first, r.last_window = last, r.width = width, r.n_out = (uint32_t)n_out;
    r.n_services = c.n_services, r.hll_p = c.hll_p;
    r.hll_hist = hist.data(), r.distinct = distinct.data(), r.error_spans = error_spans.data();
    r.n_keys = n_keys, r.errors = errors.data();
  }
};

struct top_holder {
  sa_top_result r;
  std::vector<uint64_t> keys, errors;
  // the columns sized for n rows, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, uint32_t k, uint32_t n) {
    keys.resize(n), errors.resize(n);
    r.first_window = first, r.last_window = last, r.k = k, r.n = n;
    r.n_resident = r.n_matched = r.error_spans = 0;
    r.key_hash = keys.data(), r.errors = errors.data();
  }
};

struct movers_holder {
  sa_movers_result r;
  std::vector<uint64_t> keys, baseline, current;
  std::vector<int64_t> score;
  // the columns sized for n rows, and r pointing at them; range: base first, base last, current first, current last
  __attribute__((visibility("hidden"))) void shape(const uint64_t range[4], uint32_t k, uint32_t n, uint32_t flags) {
    keys.resize(n), score.resize(n), baseline.resize(n), current.resize(n);
    r.base_first = range[0], r.base_last = range[1], r.cur_first = range[2], r.cur_last = range[3];
    r.k = k, r.n = n, r.flags = flags, r.pad = 0;
    r.n_resident = r.n_matched = r.error_spans_base = r.error_spans_cur = 0;
    r.key_hash = keys.data(), r.score = score.data(), r.baseline = baseline.data(), r.current = current.data();
  }
};

struct error_onset_holder {
  sa_error_onset_result r;
  std::vector<uint64_t> keys, onset, before, after;
  std::vector<int64_t> score;
  // the columns sized for n rows, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, uint32_t k, uint32_t n, uint32_t flags) {
    keys.resize(n), onset.resize(n), score.resize(n), before.resize(n), after.resize(n);
    r.first_window = first, r.last_window = last, r.k = k, r.n = n, r.flags = flags, r.pad = 0;
    r.n_resident = r.n_eligible = r.n_matched = r.error_spans = 0;
    r.key_hash = keys.data(), r.onset_window = onset.data(), r.score = score.data();
    r.errors_before = before.data(), r.errors_after = after.data();
  }
};

struct overlap_holder {
  sa_overlap_result r;
  std::vector<uint32_t> services, hist, pair_hist;
  std::vector<double> distinct, union_est, shared;
  // the columns sized for the selection sel of an engine of precision p, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, const std::vector<uint32_t> &sel,
                                                   uint32_t p) {
    const size_t n = sel.size(), np = n * (n - 1) / 2;
    services = sel;
    hist.resize(n * SA_HLL_HIST_BINS), distinct.resize(n);
    pair_hist.resize(np * SA_HLL_HIST_BINS), union_est.resize(np), shared.resize(np);
    r.first_window = first, r.last_window = last, r.n_sel = (uint32_t)n, r.n_pairs = (uint32_t)np;
    r.hll_p = p, r.pad = 0;
    r.services = services.data(), r.hll_hist = hist.data(), r.distinct = distinct.data();
    r.pair_hist = pair_hist.data(), r.union_est = union_est.data(), r.shared = shared.data();
  }
};

struct latency_holder {
  sa_latency_result r;
  std::vector<uint32_t> services, q_ppm;
  std::vector<uint64_t> count, q_ns, hist;
  std::vector<uint8_t> q_bin;
  // the columns sized for outputs first..last of the selection sel and n_q quantiles (hist: with
  // SA_LAT_HIST), and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, uint32_t width,
                                                   const std::vector<uint32_t> &sel, const uint32_t *ppm, uint32_t n_q,
                                                   uint32_t flags) {
    const size_t n_out = (size_t)(last - first + 1), rows = n_out * sel.size();
    services = sel;
    q_ppm.assign(ppm, ppm + n_q);
    count.resize(rows), q_bin.resize(rows * n_q), q_ns.resize(rows * n_q);
    if (flags & SA_LAT_HIST) hist.resize(rows * SA_LAT_BINS);
    r.first_window = first, r.last_window = last, r.width = width, r.n_out = (uint32_t)n_out;
    r.n_sel = (uint32_t)sel.size(), r.n_q = n_q;
    r.services = services.data(), r.q_ppm = q_ppm.data(), r.count = count.data();
    r.q_bin = q_bin.data(), r.q_ns = q_ns.data();
    r.hist = (flags & SA_LAT_HIST) ? hist.data() : nullptr;
  }
};

struct latency_movers_holder {
  sa_latency_movers_result r;
  std::vector<uint32_t> q_ppm, services;
  std::vector<int32_t> shift;
  std::vector<uint64_t> count_base, count_cur, q_ns_base, q_ns_cur;
  std::vector<uint8_t> q_bin_base, q_bin_cur;
  // the columns sized for n rows of n_q quantiles, and r pointing at them; range: base first, base last,
  // current first, current last
  __attribute__((visibility("hidden"))) void shape(const uint64_t range[4], uint32_t k, uint32_t n, const uint32_t *ppm,
                                                   uint32_t n_q, uint32_t flags, uint64_t n_services) {
    q_ppm.assign(ppm, ppm + n_q);
    services.resize(n), shift.resize(n), count_base.resize(n), count_cur.resize(n);
    q_bin_base.resize((size_t)n * n_q), q_bin_cur.resize((size_t)n * n_q);
    q_ns_base.resize((size_t)n * n_q), q_ns_cur.resize((size_t)n * n_q);
    r.base_first = range[0], r.base_last = range[1], r.cur_first = range[2], r.cur_last = range[3];
    r.k = k, r.n = n, r.n_q = n_q, r.flags = flags;
    r.n_services = n_services, r.n_eligible = r.n_matched = r.spans_base = r.spans_cur = 0;
    r.q_ppm = q_ppm.data(), r.services = services.data(), r.shift = shift.data();
    r.count_base = count_base.data(), r.count_cur = count_cur.data();
    r.q_bin_base = q_bin_base.data(), r.q_bin_cur = q_bin_cur.data();
    r.q_ns_base = q_ns_base.data(), r.q_ns_cur = q_ns_cur.data();
  }
};

struct slo_holder {
  sa_slo_result r;
  std::vector<uint32_t> services, widths, limit_ppm;
  std::vector<uint64_t> threshold_ns, effective_ns;
  std::vector<uint8_t> threshold_bin;
  // The device's answers as it lays them out, so that one copy brings them: total and slow [cells] u64
  // each, cells = n_out * n_widths * n_sel, then alert_outputs [n_sel] u32 in alert_words words and
  // burning [n_out][n_sel] u8 in burn_words words.
  std::vector<uint64_t> answers;
  size_t cells = 0, alert_words = 0, burn_words = 0;
  // the columns sized for outputs first..last of the selection sel and n_widths widths, and r pointing at
  // them; bins [sel.size()]: every threshold's bin
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, const uint32_t *w,
                                                   const uint32_t *limits, uint32_t n_widths,
                                                   const std::vector<uint32_t> &sel, const uint64_t *thresholds,
                                                   const std::vector<uint8_t> &bins, uint64_t min_count) {
    const size_t n_out = (size_t)(last - first + 1), n_sel = sel.size();
    services = sel, threshold_bin = bins;
    widths.assign(w, w + n_widths), limit_ppm.assign(limits, limits + n_widths);
    threshold_ns.assign(thresholds, thresholds + n_sel), effective_ns.resize(n_sel);
    cells = n_out * n_widths * n_sel, alert_words = (n_sel + 1) / 2, burn_words = (n_out * n_sel + 7) / 8;
    answers.resize(2 * cells + alert_words + burn_words);
    r.first_window = first, r.last_window = last, r.n_out = (uint32_t)n_out, r.n_sel = (uint32_t)n_sel;
    r.n_widths = n_widths, r.pad = 0, r.min_count = min_count;
    r.services = services.data(), r.widths = widths.data(), r.limit_ppm = limit_ppm.data();
    r.threshold_ns = threshold_ns.data(), r.threshold_bin = threshold_bin.data(), r.effective_ns = effective_ns.data();
    r.total = answers.data(), r.slow = r.total + cells;
    r.alert_outputs = reinterpret_cast<const uint32_t *>(r.slow + cells);
    r.burning = reinterpret_cast<const uint8_t *>(r.slow + cells + alert_words);
  }
};

struct onset_holder {
  sa_onset_result r;
  std::vector<uint32_t> services;
  std::vector<int32_t> delta_ppm;
  std::vector<uint8_t> threshold_bin;
  std::vector<uint64_t> onset_window, effective_ns, total_before, slow_before, total_after, slow_after;
  // the columns sized for n rows, and r pointing at them
  __attribute__((visibility("hidden"))) void shape(uint64_t first, uint64_t last, uint32_t k, uint32_t n, uint32_t flags,
                                                   uint32_t q_ppm, uint64_t min_count, uint64_t n_services) {
    services.resize(n), delta_ppm.resize(n), threshold_bin.resize(n), onset_window.resize(n), effective_ns.resize(n);
    total_before.resize(n), slow_before.resize(n), total_after.resize(n), slow_after.resize(n);
    r.first_window = first, r.last_window = last, r.k = k, r.n = n, r.flags = flags, r.q_ppm = q_ppm;
    r.min_count = min_count, r.n_services = n_services, r.n_eligible = r.n_matched = r.spans = 0;
    r.services = services.data(), r.onset_window = onset_window.data(), r.delta_ppm = delta_ppm.data();
    r.threshold_bin = threshold_bin.data(), r.effective_ns = effective_ns.data();
    r.total_before = total_before.data(), r.slow_before = slow_before.data();
    r.total_after = total_after.data(), r.slow_after = slow_after.data();
  }
};

struct sketch_holder {
  sa_sketch_result r;
  std::vector<uint8_t> hll;
  std::vector<uint32_t> cms;
  // r: window window_id of an engine with config c, pointing at the (sized) vectors
  __attribute__((visibility("hidden"))) void wire(uint64_t window_id, const sa_config &c) {
    r.window_id = window_id, r.n_services = c.n_services, r.hll_p = c.hll_p, r.hll = hll.data();
    r.cms_d = c.cms_d, r.cms_w = c.cms_w, r.cms = cms.data();
  }
};
