// engine_read.cpp -- the read side of the engine that is not a query over the
// window ring: flush and compaction, key reclamation, stats, sa_bind_ids, the
// probes, one window's sketches (sa_window_read, _export, _advance), the merge
// hooks (sa_export_keys, sa_gather_dense), sa_debug_stamps, the engine group's
// flush-time hooks (sa_grp), and what every read shares with engine_window.cpp
// and engine_latency.cpp (sa_engine.h): begin_read, the stream hops,
// fold_errslab.  Every call here joins the launches in flight onto the engine
// stream first.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "sa_engine.h"
#include "sa_group_hooks.h"
#include "sa_results.h"

int begin_read(sa_engine *e) {
  if (int rc = set_dev(e)) return rc;
  return join_checked(e);
}

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

int fold_errslab(sa_engine *e, uint64_t ws, hipStream_t s) {
  if (!e->small.errslab) return SA_OK;
  SA_HIP(e, sa::launch_reduce_errslab(e->small.errslab, e->G * e->order.nsets, (uint64_t)e->cfg.n_windows * e->cap, ws,
                                      e->log2cap, e->errcnt + ws * e->cap, s));
  return SA_OK;
}

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

double unit_div(const sa_engine *e) { return e->cfg.unit == SA_UNIT_S ? 1e9 : 1e6; }

bool resident(const sa_engine *e, uint64_t w) {
  return w >= e->win_base && w - e->win_base < e->cfg.n_windows;
}

int read_stats(sa_engine *e, uint64_t out[sa::kNumStats]) {
  SA_HIP(e, hipMemcpyAsync(out, e->stats, sa::kNumStats * 8, hipMemcpyDeviceToHost, e->stream));
  SA_HIP(e, hipStreamSynchronize(e->stream));
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

}  // namespace

namespace sa_grp {
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
  if (b.bind_cap < n) {  // (the indices and the hashes: the two halves of one allocation)
    uint64_t both = 2 * b.bind_cap;
    const int rc = grow(e, b.bind_buf, both, 2 * std::max<uint64_t>(n, 1u << 16), "sa_bind_ids: staging hipMalloc failed");
    b.bind_cap = both / 2;
    if (rc) return rc;
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
