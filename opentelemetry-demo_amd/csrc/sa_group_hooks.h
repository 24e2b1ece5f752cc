// sa_group_hooks.h -- internal (not in the C-ABI): asynchronous forms of the
// engine's merge hooks for the engine group (spanagg_group.cpp), so a flush or
// a window query of n members waits once per phase instead of once per member
// per call.  The flush-time hooks are engine_read.cpp's, a window query's
// export and finish halves engine_window.cpp's and engine_latency.cpp's; the
// queries' argument rules are sa_query_args.h's.  Host outputs must be
// page-locked (the copies are asynchronous); every call orders `s` after the
// engine's earlier work.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "spanagg.h"

namespace sa_grp {
// sa_export_keys without the wait: the resident keys with a non-zero delta
// into d_keys (capacity cap); *h_n (pinned) = their count and *h_dropped
// (pinned) = the engine's dropped-span counter, once `s` passes this point
int export_keys_async(sa_engine *e, uint64_t *d_keys, uint64_t cap, uint64_t *h_n, uint64_t *h_dropped,
                      hipStream_t s);
// the flush-time reclamation decision's key count: *h_n (pinned) = resident
// keys, once the engine stream passes this point
int count_keys_async(sa_engine *e, uint64_t *h_n);
// empties the key table on the engine stream (after its window error counts
// are folded into the count-min cells), without waiting: the reclamation
// sa_reclaim_keys does once count_keys_async's count is over the threshold
int reclaim_async(sa_engine *e);
// the reclamation threshold of this engine's table (sa_reclaim_keys' policy)
bool over_reclaim_threshold(const sa_engine *e, uint64_t n_keys);
// waits for the engine stream
int sync_stream(sa_engine *e);
// key-table slots (sa_stats.table_capacity without a device read)
uint64_t table_capacity(const sa_engine *e);
// sa_window_range's device part for one member, without the wait: every
// window of first..last folded, then d_hll [n_services][2^p] = their registers
// max-merged (nullptr: the cells only) and d_cms [d][w] = their cells summed
// (u64), on `s`.  SA_ERANGE as sa_window_range.
int window_range_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, uint64_t *d_cms,
                              hipStream_t s);
// the rest of a group's range query, on member 0 (`e`, whose device holds the
// merged d_hll and d_cms) and on `s`: the histogram of d_hll, the point
// queries on d_cms, the copies and the wait.  keys, flags and *out as
// sa_window_range.
int window_range_finish(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *d_hll, const uint64_t *d_cms,
                        const uint64_t *keys, uint64_t n_keys, uint32_t flags, hipStream_t s, sa_range_result **out);
// sa_window_overlap's merge for one member, without the wait: d_hll
// [n_services][2^p] = the registers of windows first..last max-merged, on `s`
// (no cell is folded or summed: only the registers are read).  SA_ERANGE as
// sa_window_range.
int window_overlap_export_async(sa_engine *e, uint64_t first, uint64_t last, uint8_t *d_hll, hipStream_t s);
// the rest of a group's overlap query, on member 0 (`e`, whose device holds
// the members' merged d_hll [n_services][2^p]) and on `s`: the selected rows
// gathered with their histograms, the pairs' histograms, the copies, the wait
// and the estimates.  sel: sa_args::overlap_select's.
int window_overlap_finish(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *d_hll,
                          const std::vector<uint32_t> &sel, hipStream_t s, sa_overlap_result **out);
// sa_window_latency's sums stage for one member, without the wait: d_sums
// [n_out][sel.size()][SA_LAT_BINS] = the rows of the selected services summed
// over each output's windows, on `s`.  sel (sa_args::latency_args') must stay until `s`
// has been waited for.  SA_ESTATE without the option, SA_ERANGE as
// sa_window_latency.
int window_latency_export_async(sa_engine *e, uint64_t first, uint64_t last, uint32_t width,
                                const std::vector<uint32_t> &sel, uint64_t *d_sums, hipStream_t s);
// the rest of a group's latency query, on member 0 (`e`, whose device holds
// the members' summed d_sums) and on `s`: the counts and quantile bins, the
// copies, the wait and the bins' bounds.
int window_latency_finish(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const std::vector<uint32_t> &sel,
                          const uint32_t *q_ppm, uint32_t n_q, uint32_t flags, const uint64_t *d_sums, hipStream_t s,
                          sa_latency_result **out);
// sa_window_latency_movers' sums stage for one member, without the wait:
// d_sums [2][n_services][SA_LAT_BINS] = every service's rows summed over
// range[0]..range[1] (the baseline) and over range[2]..range[3] (the current
// range), on `s`.  SA_ESTATE without the option, SA_ERANGE as sa_window_range.
int window_latency_movers_export_async(sa_engine *e, const uint64_t range[4], uint64_t *d_sums, hipStream_t s);
// the rest of the query, on `e` (a group's member 0, whose device holds the
// members' summed d_sums) and on `s`: the scores, the select and the sort, the
// selected rows, the copies, the wait and the bins' bounds.  The arguments
// (sa_args::latency_movers_args passed them) and *out as sa_window_latency_movers.
int window_latency_movers_finish(sa_engine *e, const uint64_t range[4], uint32_t k, uint64_t min_count,
                                 uint32_t min_shift, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                                 const uint64_t *d_sums, hipStream_t s, sa_latency_movers_result **out);
// sa_window_slo's pairs stage for one member, without the wait: d_pairs
// [sel.size()][n_cov][2], n_cov = last - first + max(widths): per selected
// service and covered window first - max(widths) + 1 .. last the row's spans
// and those in bins above bins[i] (= sa_latency_bin of the service's
// threshold), on `s`.  sel (sa_args::slo_args') and bins must stay until `s`
// has been waited for.  SA_ESTATE without the option, SA_ERANGE as sa_window_slo.
int window_slo_export_async(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, uint32_t n_widths,
                            const std::vector<uint32_t> &sel, const std::vector<uint8_t> &bins, uint64_t *d_pairs,
                            hipStream_t s);
// the rest of the query, on `e` (a group's member 0, whose device holds the
// members' summed d_pairs) and on `s`: the prefix sums, every width's sums,
// the verdicts, the copies and the wait.  The arguments (sa_args::slo_args
// passed them; threshold_ns parallel to sel) and *out as sa_window_slo.
int window_slo_finish(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths, const uint32_t *limit_ppm,
                      uint32_t n_widths, const std::vector<uint32_t> &sel, const uint64_t *threshold_ns,
                      uint64_t min_count, const uint64_t *d_pairs, hipStream_t s, sa_slo_result **out);
// sa_window_latency_onset's pooled sums for one member, without the wait:
// d_sums [n_services][SA_LAT_BINS] = every service's rows summed over
// first..last, on `s`.  SA_ESTATE without the option, SA_ERANGE as
// sa_window_range.
int window_onset_sums_export_async(sa_engine *e, uint64_t first, uint64_t last, uint64_t *d_sums, hipStream_t s);
// its pairs stage for one member, without the wait: the member's threshold
// bins -- bins [n_services] (host; must stay until `s` has been waited for),
// or with bins == nullptr the bins of quantile q_ppm of d_sums (the members'
// summed rows, on this member's device) -- then d_pairs [n_services][n_cov]
// [2], n_cov = last - first + 1, cut at them, on `s`.  Errors as the sums'.
int window_onset_pairs_export_async(sa_engine *e, uint64_t first, uint64_t last, const uint8_t *bins,
                                    const uint64_t *d_sums, uint32_t q_ppm, uint64_t *d_pairs, hipStream_t s);
// the rest of the query, on `e` (a group's member 0, whose device holds the
// members' summed d_pairs and, from its own pairs stage, the threshold bins)
// and on `s`: the scan, the select and the sort, the selected rows, the copies
// and the wait.  The arguments (sa_args::onset_args passed them; pooled: no
// threshold_ns was given) and *out as sa_window_latency_onset.
int window_onset_finish(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint32_t q_ppm, bool pooled,
                        uint64_t min_count, uint32_t min_delta_ppm, uint32_t flags, const uint64_t *d_pairs,
                        hipStream_t s, sa_onset_result **out);
// What one engine's heavy-hitter scan leaves on the host once its stream
// passes the copies: head = the matches, the resident keys, the largest
// estimate, error_spans; rows [k] = (estimate, key) pairs, the first
// min(k, head[0]) of them the engine's answer in order.
struct TopHost {
  unsigned long long head[4] = {};
  std::vector<ulonglong2> rows;
};
// sa_window_top's device part for one member against the merged cells d_cms
// [d][w] on its device, on `s`, without the wait: fills *out (which must stay
// until `s` has been waited for).  k and min_count as sa_window_top.
int window_top_async(sa_engine *e, const uint64_t *d_cms, uint32_t k, uint64_t min_count, hipStream_t s, TopHost *out);
// The sa_top_result of n_members scans (each waited for): one member's rows
// as they are; several members' merged -- repeats dropped, ordered by
// (estimate descending, key ascending), cut to k -- with n_resident and
// n_matched summed.  SA_ENOMEM when the result cannot be allocated.
int top_result(uint64_t first, uint64_t last, uint32_t k, const TopHost *members, uint32_t n_members,
               sa_top_result **out);
// What one engine's movers scan leaves on the host: top as TopHost with the
// score for the estimate (head[2] the largest score, head[3] the current
// range's error_spans); out [k + 1] = {the baseline's error_spans, -}, then the
// rows' (baseline, current) estimates in top.rows' order.
struct MoversHost {
  TopHost top;
  std::vector<ulonglong2> out;
};
// sa_window_movers' device part for one member against the merged cells
// d_base and d_cur [d][w] on its device (the sums of nb and nc windows), on
// `s`, without the wait: fills *out (which must stay until `s` has been waited
// for).  k, min_score and flags as sa_window_movers.
int window_movers_async(sa_engine *e, const uint64_t *d_base, const uint64_t *d_cur, uint64_t nb, uint64_t nc,
                        uint32_t k, uint64_t min_score, uint32_t flags, hipStream_t s, MoversHost *out);
// The sa_movers_result of n_members scans (each waited for), merged as
// top_result merges; range: base first, base last, current first, current
// last.  SA_ENOMEM when the result cannot be allocated.
int movers_result(const uint64_t range[4], uint32_t k, uint32_t flags, const MoversHost *members, uint32_t n_members,
                  sa_movers_result **out);
// sa_window_error_onset's export for one member, without the wait: every
// window of first..last folded, then d_win [n][d * w] = the cells of window
// first + j in row j (u64, unwrapped; n = last - first + 1), on `s`.  SA_ERANGE
// as sa_window_range.
int window_cells_export_async(sa_engine *e, uint64_t first, uint64_t last, uint64_t *d_win, hipStream_t s);
// What one engine's error-onset scan leaves on the host: top as TopHost with
// the best D for the estimate; out = {the eligible keys, -}, then the rows'
// (t, B, A) in top.rows' order (sa::ErrOnsetOut's head and first k rows).
struct ErrOnsetHost {
  TopHost top;
  std::vector<unsigned long long> out;
};
// sa_window_error_onset's device part for one member against the merged
// windows d_win [n][d * w] on its device, on `s`, without the wait: fills *out
// (which must stay until `s` has been waited for).  k, min_count, min_score and
// flags as sa_window_error_onset.
int window_error_onset_async(sa_engine *e, const uint64_t *d_win, uint32_t n, uint32_t k, uint64_t min_count,
                             uint64_t min_score, uint32_t flags, hipStream_t s, ErrOnsetHost *out);
// The sa_error_onset_result of n_members scans (each waited for), merged as
// top_result merges.  SA_ENOMEM when the result cannot be allocated.
int error_onset_result(uint64_t first, uint64_t last, uint32_t k, uint32_t flags, const ErrOnsetHost *members,
                       uint32_t n_members, sa_error_onset_result **out);
}  // namespace sa_grp
