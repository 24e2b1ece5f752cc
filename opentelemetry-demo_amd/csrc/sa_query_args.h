// sa_query_args.h -- the window queries' argument rules, one copy for the
// engine (engine_window.cpp, engine_latency.cpp) and the engine group
// (spanagg_group.cpp).  Plain host C++ (no HIP header), so a stand-alone
// program can run them (tests/test_query_args_host.py).  Every rule returns
// nullptr when the arguments pass, else what is wrong; the caller puts the
// query's name in front and picks the code: SA_ERANGE for span, SA_ESTATE for
// latency_option, SA_EINVAL for the rest.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "spanagg.h"

#pragma GCC visibility push(hidden)  // internal to the library
namespace sa_args {

// Outputs first..last, each over the `width` windows that end at it, on a ring
// that holds windows win_base .. win_base + n_windows - 1: every covered
// window, first - width + 1 .. last, must be resident.  The range queries pass
// width 1.
inline const char *span(uint64_t first, uint64_t last, uint32_t width, uint64_t win_base, uint32_t n_windows) {
  const auto resident = [&](uint64_t w) { return w >= win_base && w - win_base < n_windows; };
  if (first > last) return "first > last";
  if (width == 0 || width > n_windows) return "a width outside 1..n_windows";
  if (first < width - 1 || !resident(first - (width - 1)) || !resident(last)) return "a covered window is not resident";
  return nullptr;
}

inline const char *top_k(uint32_t k) { return k == 0 || k > SA_TOP_MAX_K ? "k outside 1..SA_TOP_MAX_K" : nullptr; }

// known == 0: the query takes no flag yet
inline const char *flags(uint32_t flags, uint32_t known) {
  if (flags & ~known) return known ? "unknown flag bits" : "flags are reserved (0)";
  return nullptr;
}

inline const char *keys(const uint64_t *keys, uint64_t n_keys) {
  return n_keys && !keys ? "n_keys != 0 with null keys" : nullptr;
}

inline const char *q_ppm(const uint32_t *q_ppm, uint32_t n_q) {
  if (n_q == 0 || n_q > SA_LAT_MAX_Q || !q_ppm) return "n_q outside 1..SA_LAT_MAX_Q or null q_ppm";
  for (uint32_t i = 0; i < n_q; ++i)
    if (q_ppm[i] == 0 || q_ppm[i] > 1000000u) return "a q_ppm outside 1..1000000";
  return nullptr;
}

// options: the sa_config's the engine or the group was created with
inline const char *latency_option(uint32_t options) {
  return options & SA_OPT_WINDOW_LATENCY ? nullptr : "not created with SA_OPT_WINDOW_LATENCY";
}

// A selection of services out of n_services, at most max_sel of them: *sel =
// the ids in the caller's order (services == nullptr with n_sel == 0: every id).
inline const char *select_services(uint32_t n_services, const uint32_t *services, uint32_t n_sel, uint32_t max_sel,
                                   std::vector<uint32_t> *sel) {
  sel->clear();
  if (!services) {
    if (n_sel) return "n_sel != 0 with null services";
    if (n_services > max_sel) return "every service asked for on an engine with more services than a selection holds";
    for (uint32_t i = 0; i < n_services; ++i) sel->push_back(i);
    return nullptr;
  }
  if (n_sel == 0) return "an empty selection";
  if (n_sel > max_sel) return "more services than a selection holds (a repeated id, or past SA_OVERLAP_MAX_SERVICES)";
  std::vector<bool> seen(n_services, false);
  for (uint32_t i = 0; i < n_sel; ++i) {
    if (services[i] >= n_services) return "a service id at or past n_services";
    if (seen[services[i]]) return "a repeated service id";
    seen[services[i]] = true;
    sel->push_back(services[i]);
  }
  return nullptr;
}

// sa_window_overlap's selection: at most SA_OVERLAP_MAX_SERVICES ids
inline const char *overlap_select(uint32_t n_services, const uint32_t *services, uint32_t n_sel,
                                  std::vector<uint32_t> *sel) {
  return select_services(n_services, services, n_sel, SA_OVERLAP_MAX_SERVICES, sel);
}

// sa_window_latency's arguments, the span apart: *sel as overlap_select's, of
// up to n_services ids
inline const char *latency_args(uint32_t n_services, const uint32_t *services, uint32_t n_sel, const uint32_t *q,
                                uint32_t n_q, uint32_t flag_bits, std::vector<uint32_t> *sel) {
  sel->clear();
  if (const char *bad = flags(flag_bits, SA_LAT_HIST)) return bad;
  if (const char *bad = q_ppm(q, n_q)) return bad;
  return select_services(n_services, services, n_sel, n_services, sel);
}

// its size rule, once the span is known to be resident: n_out * n_sel <= 2^20
// (2^16 with SA_LAT_HIST)
inline const char *latency_rows(uint64_t n_out, uint64_t n_sel, uint32_t flag_bits) {
  if (n_out * n_sel > ((flag_bits & SA_LAT_HIST) ? 1ull << 16 : 1ull << 20))
    return "n_out * n_sel above 2^20 (2^16 with SA_LAT_HIST)";
  return nullptr;
}

// sa_window_latency_movers' arguments, the ranges apart
inline const char *latency_movers_args(uint32_t k, const uint32_t *q, uint32_t n_q, uint32_t flag_bits) {
  if (const char *bad = top_k(k)) return bad;
  if (const char *bad = flags(flag_bits, SA_LATMOV_FALL)) return bad;
  return q_ppm(q, n_q);
}

// sa_window_slo's arguments, the spans apart: 1..SA_SLO_MAX_WIDTHS widths (any
// order, repeats pass) with a limit in 0..10^6 each, a threshold (any u64) a
// selected service, no flag; *sel as latency_args'
inline const char *slo_args(uint32_t n_services, const uint32_t *widths, const uint32_t *limit_ppm, uint32_t n_widths,
                            const uint32_t *services, uint32_t n_sel, const uint64_t *threshold_ns,
                            uint32_t flag_bits, std::vector<uint32_t> *sel) {
  sel->clear();
  if (const char *bad = flags(flag_bits, 0)) return bad;
  if (n_widths == 0 || n_widths > SA_SLO_MAX_WIDTHS || !widths || !limit_ppm)
    return "n_widths outside 1..SA_SLO_MAX_WIDTHS or null widths or limit_ppm";
  for (uint32_t w = 0; w < n_widths; ++w)
    if (limit_ppm[w] > 1000000u) return "a limit_ppm above 1000000";
  if (!threshold_ns) return "null threshold_ns";
  return select_services(n_services, services, n_sel, n_services, sel);
}

// its span rule: every width passes `span` against first..last, so every
// window first - max(widths) + 1 .. last is resident
inline const char *slo_span(uint64_t first, uint64_t last, const uint32_t *widths, uint32_t n_widths, uint64_t win_base,
                            uint32_t n_windows) {
  for (uint32_t w = 0; w < n_widths; ++w)
    if (const char *bad = span(first, last, widths[w], win_base, n_windows)) return bad;
  return nullptr;
}

// its size rule, once the spans are known to be resident: n_out * n_sel <= 2^20
inline const char *slo_rows(uint64_t n_out, uint64_t n_sel) {
  return n_out * n_sel > 1ull << 20 ? "n_out * n_sel above 2^20" : nullptr;
}

// sa_window_latency_onset's arguments, the range apart: k, the one flag, and
// the threshold's two forms -- given (threshold_ns != nullptr, one a service,
// any u64: q_ppm must be 0) or pooled (q_ppm in 1..10^6)
inline const char *onset_args(uint32_t k, uint32_t q, const uint64_t *threshold_ns, uint32_t flag_bits) {
  if (const char *bad = top_k(k)) return bad;
  if (const char *bad = flags(flag_bits, SA_ONSET_FALL)) return bad;
  if (threshold_ns) return q ? "q_ppm != 0 with threshold_ns given" : nullptr;
  return q == 0 || q > 1000000u ? "null threshold_ns with q_ppm outside 1..1000000" : nullptr;
}

// sa_window_error_onset's arguments, the range apart: k and the one flag
// (min_count and min_score: any u64)
inline const char *error_onset_args(uint32_t k, uint32_t flag_bits) {
  if (const char *bad = top_k(k)) return bad;
  return flags(flag_bits, SA_ERROR_ONSET_FALL);
}

}  // namespace sa_args
#pragma GCC visibility pop
