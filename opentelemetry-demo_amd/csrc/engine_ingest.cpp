// engine_ingest.cpp -- the launch side of the engine: one common frame
// (ingest_launch) around a launcher per path, the graph form of k small-table
// launches, host batches through the staging slots, and the joins that order
// readers after the launches in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "sa_engine.h"
#include "spanagg_diag.h"

using sa::IngestParams;
using sa::Path;

namespace {

constexpr uint64_t kSlabLimit = 1ULL << 31;  // per-workgroup spans between slab reductions
// exponential slab path: what the ingest kernel hands the counting pass per
// span (expo_rec_mode): 0 the key slot (the pass reads both times too), 1 an
// 8-B span record (slot | duration), 2 an index record (slot | scale | bucket
// index, ixrec_of) -- DESIGN.md section 4
constexpr int kExpoRecMode = 2;
long g_aggregates = 0;  // aggregate launches of the process (laboratory build: SPANAGG_FAIL_AGG)

// The aggregate of record set k alone (pend < 0), or of the pending set and k
// together (the pending set's records first), on `as` after both scatters.
int bt_launch_aggregate(sa_engine *e, int pend, const IngestParams &Pp, int k, const IngestParams &Pk, hipStream_t as) {
  sa_engine::Binned &b = e->binned;
  IngestParams A = pend >= 0 ? Pp : Pk;
  if (pend >= 0) {
    A.bt_rec2 = Pk.bt_rec;
    A.bt_cnt2 = Pk.bt_cnt;
    A.bt_grid2 = Pk.bt_grid;
    A.bt_region2 = Pk.bt_region;
  }
  for (int j : {pend, k})
    if (j >= 0) SA_HIP(e, hipStreamWaitEvent(as, b.ev_scat[j], 0));
  // laboratory build: SPANAGG_FAIL_AGG=n fails the n-th aggregate launch of
  // the process (tests of the pending-set error path)
  if (lab().fail_agg > 0 && ++g_aggregates == lab().fail_agg)
    return fail(e, SA_EDEVICE, "aggregate launch: injected failure");
  if (hipError_t st = e->dense() ? sa::launch_dn_aggregate(A, as) : sa::launch_bt_aggregate(A, as); st != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("aggregate launch: ") + hipGetErrorString(st));
  for (int j : {pend, k})
    if (j >= 0) {
      SA_HIP(e, hipEventRecord(b.ev_agg[j], as));
      b.agg_used[j] = true;
    }
  return SA_OK;
}

// Every launch of an aggregate that takes a pending record set goes through
// here: the pending set belongs to an ingest that already returned SA_OK, so a
// failure is kept (sticky_rc) and returned by every later read instead of
// results without those records.
int bt_launch_with_pending(sa_engine *e, const IngestParams &Pk, int k, hipStream_t as) {
  const int pend = e->binned.pend;
  e->binned.pend = -1;
  const int rc = bt_launch_aggregate(e, pend, e->binned.pend_P, k, Pk, as);
  if (rc && pend >= 0 && !e->binned.sticky_rc) e->binned.sticky_rc = rc;
  return rc;
}

int bt_aggregate_pending(sa_engine *e) {
  sa_engine::Binned &b = e->binned;
  if (!sa::binned_like(e->path) || b.pend < 0) return SA_OK;
  const int k = b.pend;
  b.pend = -1;
  const int rc = bt_launch_aggregate(e, -1, b.pend_P, k, b.pend_P, b.agg_stream);
  if (rc && !b.sticky_rc) b.sticky_rc = rc;
  return rc;
}

// Orders a stream after every outstanding launch: wait(event) for each slab
// set's last user (unless it ran on `s` itself) and the binned path's
// aggregates; stops at the first wait that returns non-zero.
template <class Wait>
int join_onto(sa_engine *e, hipStream_t s, Wait wait) {
  for (uint32_t i = 0; i < e->order.nsets; ++i)
    if (e->order.set_stream[i] && e->order.set_stream[i] != s)
      if (int rc = wait(e->order.ev_set[i])) return rc;
  for (int k = 0; k < sa_engine::Binned::kSets; ++k)
    if (e->binned.agg_used[k])
      if (int rc = wait(e->binned.ev_agg[k])) return rc;
  return SA_OK;
}

// The exponential slab path's span words (kExpoRecMode; laboratory build:
// SPANAGG_XREC=0 / 1 / 2 picks, for A/B runs); slab counting only
int expo_rec_mode(const sa_engine *e) {
  if (e->path != Path::ExpoSmall || !e->expo.xc_ne) return 0;
  const int knob = lab().xrec;
  return knob >= 0 && knob <= 2 ? knob : kExpoRecMode;
}

}  // namespace

// the next launch orders after whatever the caller enqueues on the engine
// stream now (ev_ctl, recorded lazily by that launch)
void join_sets(sa_engine *e) {
  // a pending binned record set is aggregated first; a failed launch is
  // kept (sticky_rc, bt_aggregate_pending) and returned by join_checked, so
  // no read goes on without it
  (void)bt_aggregate_pending(e);
  (void)join_onto(e, e->stream, [&](hipEvent_t ev) -> int {  // (a failed wait is not reported here)
    (void)hipStreamWaitEvent(e->stream, ev, 0);
    return SA_OK;
  });
  e->order.ctl_dirty = true;
}

int join_checked(sa_engine *e) {
  join_sets(e);
  return e->binned.sticky_rc;
}

int reduce_slabs(sa_engine *e, hipStream_t s) {
  if (e->path != Path::Small || e->small.slab_load == 0) return SA_OK;
  SA_HIP(e, sa::launch_reduce_slabs(e->small.slab_cnt, e->small.slab_sum, e->gcounts, e->G * e->order.nsets, e->cap,
                                    e->hist.nbk, s));
  e->small.slab_load = 0;
  return SA_OK;
}

// Binned path: launch geometry, record regions (allocated once for the
// largest launch).  Region capacity: the mean records
// per (bin, scatter workgroup) plus 4 standard deviations and 8, in whole
// 4-record chunks; records beyond it take the scatter's overflow table.
uint32_t bt_region_for(const sa_engine *e, uint64_t wg_chunk) {
  const double mu = (double)wg_chunk / sa::kPartBins;
  const uint32_t stage = e->dense() ? sa::kDnStage : sa::kBtStage;  // (dense: whole 8-record chunks)
  return ((uint32_t)std::ceil(mu + 4.0 * std::sqrt(mu) + 8.0) + stage - 1) & ~(stage - 1);
}

sa::ExpoParams expo_params(sa_engine *e, const sa_span_batch *b, uint32_t set) {
  const sa_engine::Expo &x = e->expo;
  const bool xsmall = e->path == Path::ExpoSmall;
  sa::ExpoParams E{};
  if (b) {
    E.key = b->key_hash;
    E.start = b->start_ns;
    E.end = b->end_ns;
    E.n = b->n;
  }
  E.gkeys = e->gkeys;
  E.log2cap = e->log2cap;
  E.max_probe = sa::max_probe_of(e->log2cap);
  E.cap = e->cap;
  E.hdr = x.hdr;
  E.xscale = x.xscale;
  E.buckets = x.buckets;
  E.max_size = e->cfg.exp_max_size;
  E.div = e->cfg.unit == SA_UNIT_S ? 1e9 : 1e6;
  E.log2div_q24 = sa::expo_l2d_q24(E.div);
  E.diag = lab().xc_diag;
  // (this launch's set of span slots / records and header partials)
  // (per set: n span records or u32 slots, then n long durations)
  E.slot_of = x.slot ? x.slot + 4 * (size_t)set * x.slot_cap : nullptr;
  E.span_rec = expo_rec_mode(e) == 1 ? reinterpret_cast<const unsigned long long *>(E.slot_of) : nullptr;
  E.xidx = expo_rec_mode(e) == 2 ? 1u : 0u;
  E.span_long = (E.span_rec || E.xidx) && x.slot
                    ? reinterpret_cast<const unsigned long long *>(E.slot_of) + x.slot_cap
                    : nullptr;
  E.dropped = e->stats + sa::kStatDropped;
  E.xslab = xsmall ? x.xslab + (size_t)set * e->G * e->cap : nullptr;
  // the workgroups whose header partials this launch wrote (ingest_launch's
  // grid: each writes every slot of its slab row; rows past it are stale)
  E.xG = b ? (uint32_t)std::min<uint64_t>((b->n + (uint64_t)e->block * e->spl - 1) / ((uint64_t)e->block * e->spl), e->G)
           : e->G;
  E.xc_ne = xsmall ? x.xc_ne : 0u;
  E.lcount = E.xc_ne ? x.xc_lcount : nullptr;
  E.xmeta = E.xc_ne ? reinterpret_cast<int2 *>(x.xc_lcount + e->cap) : nullptr;
  // (compact passes no batch and reads none of these)
  const uint32_t cur = x.xc_sel & 1u, nxt = cur ^ 1u;
  E.slot_of_entry = x.xc_slot_of_entry ? x.xc_slot_of_entry + (size_t)cur * x.xc_ne : nullptr;
  E.soe_next = x.xc_slot_of_entry ? x.xc_slot_of_entry + (size_t)nxt * x.xc_ne : nullptr;
  E.xent = x.xc_ent ? x.xc_ent + (size_t)cur * e->cap : nullptr;
  E.xent_next = x.xc_ent ? x.xc_ent + (size_t)nxt * e->cap : nullptr;
  if (!x.xc_sel_made) {  // the first launch: its own selection, in every counting workgroup
    E.xent = nullptr;
    E.slot_of_entry = E.soe_next;
  }
  E.xcslab = x.xcslab;
  // laboratory build: SPANAGG_XT=0 sends the counting kernel's tail to HBM
  // atomics (the earlier form), for A/B runs
  E.xt_rec = lab().xt && E.xc_ne ? x.xt_rec : nullptr;
  E.xt_off = x.xt_off;
  E.dbg = e->dbg;
  return E;
}

namespace {

// v2 small-table kernels keep u16 LDS counters for the whole launch: at most
// 65532 spans per workgroup per launch (ingest_v2_kernel has no epoch flush);
// the HBM-table kernels' workgroup ranges stay addressable by a 32-bit
// buffer offset (< 2^27 spans per workgroup per launch).
uint64_t max_spans_per_launch(const sa_engine *e) {
  switch (e->path) {
    case Path::Binned:
    case Path::Dense: return (uint64_t)e->binned.grid * sa::kBtMaxWgSpans;
    case Path::Partitioned: return sa::kPartMaxSpans;
    case Path::Small:  // (the linear-threshold kernel flushes every epoch; it keeps the v2 kernels' limit)
    case Path::ExpoSmall: return (uint64_t)e->G * sa::kMaxWgSpans;
    case Path::ExpoHbm:
    case Path::Atomic: break;
  }
  return (uint64_t)e->G << 27;
}

// Workgroup ranges of one launch of n spans (n > 0).
struct LaunchPlan {
  uint32_t grid = 0;
  uint64_t wg_chunk = 0;
  uint64_t slab_load = 0;  // what the launch adds to a workgroup's slab counters (Small)
};

LaunchPlan plan_launch(const sa_engine *e, uint64_t n) {
  LaunchPlan pl;
  const uint64_t tile = (uint64_t)e->block * e->spl;
  // each workgroup gets one contiguous range of >= one tile (kernel: wg_range)
  pl.grid = (uint32_t)std::min<uint64_t>((n + tile - 1) / tile, e->G);
  const uint64_t per = (n + pl.grid - 1) / pl.grid;
  pl.wg_chunk = (per + 3) / 4 * 4;
  if (e->path == Path::Small) pl.slab_load = pl.wg_chunk;
  return pl;
}

// Small path: folds every set into the counters before `load` more spans per
// workgroup would pass the slab cells' limit.
int make_slab_room(sa_engine *e, uint64_t load) {
  if (e->small.slab_load + load <= kSlabLimit) return SA_OK;
  if (int rc = join_checked(e)) return rc;
  return reduce_slabs(e, e->stream);
}

// Orders n launches on `s`, into the slab sets from first_set on: after the
// engine stream's work so far (ev_ctl, re-recorded after each join) and after
// the previous launch that used each set.
int order_before(sa_engine *e, hipStream_t s, uint32_t first_set, uint32_t n) {
  sa_engine::Order &o = e->order;
  if (o.ctl_dirty) {
    SA_HIP(e, hipEventRecord(o.ev_ctl, e->stream));
    o.ctl_dirty = false;
  }
  if (s != e->stream) SA_HIP(e, hipStreamWaitEvent(s, o.ev_ctl, 0));
  for (uint32_t j = 0; j < o.nsets && j < n; ++j) {
    const uint32_t set = (first_set + j) % o.nsets;
    if (o.set_stream[set] && o.set_stream[set] != s) SA_HIP(e, hipStreamWaitEvent(s, o.ev_set[set], 0));
  }
  return SA_OK;
}

// The n launches' last kernels ran on hs: marks their sets, moves on to the next.
int mark_after(sa_engine *e, hipStream_t hs, uint32_t first_set, uint32_t n, bool record = true) {
  sa_engine::Order &o = e->order;
  for (uint32_t j = 0; j < o.nsets && j < n; ++j) {
    const uint32_t set = (first_set + j) % o.nsets;
    if (record) SA_HIP(e, hipEventRecord(o.ev_set[set], hs));
    o.set_stream[set] = hs;
  }
  o.set = (first_set + n) % o.nsets;
  return SA_OK;
}

// The launch parameters of one ingest of batch b into slab set `set` (the
// workgroup ranges and tables; every path's kernels read from these).
void fill_params(sa_engine *e, const sa_span_batch *b, uint32_t set, const LaunchPlan &pl, IngestParams &P) {
  const sa::Hist &h = e->hist;
  sa_engine::Small &sm = e->small;
  const size_t srow = (h.nbk + 1) & ~1u;
  P.key = b->key_hash;
  P.start = b->start_ns;
  P.end = b->end_ns;
  P.w0 = b->trace_w0;
  P.w1 = b->trace_w1;
  P.meta = b->meta;
  P.n = b->n;
  P.wg_chunk = pl.wg_chunk;
  P.gkeys = e->gkeys;
  P.log2cap = e->log2cap;
  P.max_probe = sa::max_probe_of(e->log2cap);
  P.slab_cnt = sm.slab_cnt ? sm.slab_cnt + (size_t)set * e->G * e->cap * srow : nullptr;
  P.slab_sum = sm.slab_sum ? sm.slab_sum + (size_t)set * e->G * e->cap : nullptr;
  P.gcounts = e->gcounts;
  P.base64 = e->binned.base64;
  std::memcpy(P.thr, h.thr, sizeof h.thr);
  P.npos = h.npos;
  P.nneg = h.nneg;
  P.nbk = h.nbk;
  P.epoch_tiles = (uint32_t)(65535 / ((uint64_t)e->block * e->spl));  // (the launch's tile)
  P.hll = e->hll;
  P.cms = e->cms;
  P.errcnt = e->errcnt;
  P.errslab = sm.errslab ? sm.errslab + (size_t)set * e->G * e->cfg.n_windows * e->cap : nullptr;
  P.window_ns = e->cfg.window_ns;
  P.win_magic = UINT64_MAX / e->cfg.window_ns;
  P.win_base = e->win_base;
  P.base_ns = e->win_base * e->cfg.window_ns;  // < 2^64: checked in sa_window_advance
  P.ring_ns = (uint64_t)e->cfg.n_windows * e->cfg.window_ns;
  P.inv_window = (float)(1.0 / (double)e->cfg.window_ns);
  P.win_ok = (float)(0.5 - (double)e->cfg.n_windows * 0x1p-20);  // n_windows <= 4096: >= 0.496
  P.base_slot = (uint32_t)(e->win_base & (e->cfg.n_windows - 1));
  P.bintab = e->d_bins;
  P.win_mask = e->cfg.n_windows - 1;
  P.n_windows = e->cfg.n_windows;
  P.p = e->cfg.hll_p;
  P.n_services = e->cfg.n_services;
  P.cms_d = e->cfg.cms_d;
  P.cms_w = e->cfg.cms_w;
  P.cms_shift = 64 - sa::log2u(e->cfg.cms_w);
  P.seeds = e->d_seeds;
  P.stats = e->stats;
  P.diag = e->cfg.flags;
  P.dbg = e->dbg;
  P.hll_lb = e->hll_lb;
  P.lb_shift = e->lb_shift;
  P.lb_n = e->lb_n;  // read (and refreshed) by the v2 and binned kernels; the others ignore it
  P.lb_seq = e->lb_seq++;
  P.hll_filt = e->hll_filt;
}

int launched(sa_engine *e, hipError_t st) {
  return st == hipSuccess ? SA_OK : fail(e, SA_EDEVICE, std::string("ingest launch: ") + hipGetErrorString(st));
}

int launch_small(sa_engine *e, uint32_t grid, const IngestParams &P, hipStream_t s) {
  return launched(e, sa::launch_ingest_small(P, grid, e->lds_bytes, s, e->small_kernel, e->diag()));
}

// per-span CAS insert and atomics into the HBM rows
int launch_atomic(sa_engine *e, uint32_t grid, const IngestParams &P, hipStream_t s) {
  return launched(e, sa::launch_ingest_hbm(P, grid, s));
}

// Binned and dense: the scatter here, the aggregate on agg_stream (the
// pipeline, sa_engine::Binned).
int launch_binned(sa_engine *e, uint64_t n, IngestParams &P, hipStream_t s) {
  sa_engine::Binned &b = e->binned;
  const bool dense = e->dense();
  const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b.grid, (n + 4095) / 4096));
  P.bt_grid = grid;
  P.wg_chunk = ((n + grid - 1) / grid + 3) / 4 * 4;
  P.bt_region = bt_region_for(e, P.wg_chunk);
  if (!b.rec[0]) {
    size_t recs = (size_t)sa::kPartBins * b.grid * bt_region_for(e, sa::kBtMaxWgSpans);
    if (dense) recs = (recs + 1) / 2;  // (dense records: 8 B, half the bytes)
    for (int k = 0; k < sa_engine::Binned::kSets; ++k)
      if (dalloc(e, b.rec[k], recs, false) || dalloc(e, b.cnt[k], (size_t)b.grid * sa::kPartBins, false))
        return fail(e, SA_ENOMEM, "binned-path record buffers hipMalloc failed");
  }
  P.log2sb = b.log2sb;
  P.kmul = b.kmul;
  P.kinv = b.kinv;
  const int k = (int)b.set;
  P.bt_rec = b.rec[k];
  P.bt_cnt = b.cnt[k];
  P.bt_rec2 = nullptr;
  P.bt_cnt2 = nullptr;
  if (b.agg_used[k]) SA_HIP(e, hipStreamWaitEvent(s, b.ev_agg[k], 0));  // set k's last reader
  hipError_t st = dense ? sa::launch_dn_scatter(P, s) : sa::launch_bt_scatter(P, s);
  if (st == hipSuccess) st = hipEventRecord(b.ev_scat[k], s);
  if (int rc = launched(e, st)) return rc;
  // (laboratory build: SPANAGG_BT_PIPE=0 runs each launch's aggregate right
  // after its scatter on the caller's stream; SPANAGG_BT_PAIR=0 aggregates
  // every launch alone on the aggregate stream)
  if (!lab().bt_pipe) {
    if (int rc = bt_launch_aggregate(e, -1, P, k, P, s)) return rc;
  } else if (lab().bt_pair && b.pend < 0) {
    b.pend = k;  // aggregated with the next launch's records, or at the next join
    b.pend_P = P;
  } else {
    if (int rc = bt_launch_with_pending(e, P, k, b.agg_stream)) return rc;
  }
  b.set = (b.set + 1) % sa_engine::Binned::kSets;
  return SA_OK;
}

int launch_partitioned(sa_engine *e, uint64_t n, IngestParams &P, hipStream_t s) {
  // records per bin: 1.25x the mean plus slack; a fuller bin spills to the
  // direct path, so this bounds memory, not correctness
  const uint64_t per_bin_max = sa::kPartMaxCap;
  if (!e->part.rec) {
    const char *what = "partition buffers hipMalloc failed";
    if (dalloc(e, e->part.rec, sa::kPartBins * per_bin_max, false, what) ||
        dalloc(e, e->part.fill, sa::kPartBins, false, what))
      return SA_ENOMEM;
    // (on `s`, ahead of the scatter in stream order: a null-stream memset is
    // not ordered against a caller's non-blocking stream)
    if (hipMemsetAsync(e->part.fill, 0, sa::kPartBins * 4, s) != hipSuccess) return fail(e, SA_ENOMEM, what);
  }
  P.part_rec = e->part.rec;
  P.part_fill = e->part.fill;
  // a multiple of 4 records: staged 64-B chunks stay segment-aligned
  P.part_cap = (uint32_t)std::min<uint64_t>(
      per_bin_max, ((n + sa::kPartBins - 1) / sa::kPartBins * 5 / 4 + 64 + sa::kPartStage - 1) &
                       ~(uint64_t)(sa::kPartStage - 1));
  return launched(e, sa::launch_ingest_part(P, s));
}

// Exponential engines: the sketches (and, with a small table, the key slots
// and header partials) through an ingest kernel, then the histogram kernels
// on hs.
int launch_expo(sa_engine *e, const sa_span_batch *b, uint32_t set, uint32_t grid, IngestParams &P, hipStream_t s,
                hipStream_t &hs) {
  sa_engine::Expo &x = e->expo;
  const bool xsmall = e->path == Path::ExpoSmall;
  if (x.slot_cap < b->n) {  // (hipFree waits for the device)
    dfree(e, x.slot);
    x.slot_cap = 0;
    // (16 B per span and set: span records or u32 slots, then long durations)
    if (int rc = dalloc(e, x.slot, (size_t)e->order.nsets * b->n * 4, false, "expo slot buffer")) return rc;
    x.slot_cap = b->n;
  }
  uint32_t *slots = x.slot + 4 * (size_t)set * x.slot_cap;
  hipError_t st;
  if (xsmall) {
    // the small-table kernel in EXPO mode: sketches, key slots, header partials
    const int mode = expo_rec_mode(e);
    const bool recs = mode == 1;
    if (recs) {
      P.span_rec = reinterpret_cast<unsigned long long *>(slots);
      P.span_long = P.span_rec + x.slot_cap;
    } else {
      P.slot_of = slots;
      if (mode == 2) {
        P.xidx = x.xidx;
        P.xscale = x.xscale;
        P.l2d_q24 = sa::expo_l2d_q24(e->cfg.unit == SA_UNIT_S ? 1e9 : 1e6);
        P.span_long = reinterpret_cast<unsigned long long *>(slots) + x.slot_cap;
      }
    }
    P.xslab = x.xslab + (size_t)set * e->G * e->cap;
    st = sa::launch_ingest_expo_small(P, grid, e->lds_bytes, s);
    if (recs && x.xstream) {
      // the histogram kernels on the engine's xstream, after this ingest kernel
      hs = x.xstream;
      if (st == hipSuccess) st = hipEventRecord(x.ev_ing[set], s);
      if (st == hipSuccess) st = hipStreamWaitEvent(hs, x.ev_ing[set], 0);
    } else if (st == hipSuccess && x.last && x.last != s) {
      // on the caller's stream, after the previous launch's histogram kernels
      // (one owner of the headers and buckets at a time)
      st = hipStreamWaitEvent(s, x.ev_expo, 0);
    }
  } else {
    // sketches (and the zero-key / service / window counters) through the
    // HBM-table kernel with its RED part off
    P.diag |= SA_DIAG_NO_RED;
    st = sa::launch_ingest_hbm(P, grid, s);
  }
  // then the histogram kernels
  if (st == hipSuccess) st = sa::launch_expo_ingest(expo_params(e, b, set), hs);
  if (st == hipSuccess && xsmall && x.xc_ne) {  // (the next launch counts with this one's selection)
    x.xc_sel ^= 1u;
    x.xc_sel_made = true;
  }
  if (st == hipSuccess && x.ev_expo) {
    st = hipEventRecord(x.ev_expo, hs);
    x.last = hs;
  }
  return launched(e, st);
}

// SA_OPT_WINDOW_LATENCY: the latency kernel over the launch's batch, with the
// launch's own parameters (the same ring base and window fields).  Workgroups
// of whole 4,096-span tiles, at most the engine's resident round; a range so
// long that an LDS cell could wrap takes the HBM form.
int launch_latency(sa_engine *e, uint64_t n, const IngestParams &P, hipStream_t s) {
  const sa_engine::Latency &L = e->lat;
  if (!L.ring) return SA_OK;
  const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 4095) / 4096, L.grid_max);
  const uint64_t chunk = ((n + grid - 1) / grid + 3) / 4 * 4;
  return launched(e, sa::launch_lat_ingest(P, L.ring, grid, chunk, chunk >> 32 ? 0 : L.k_slots, s));
}

// One launch of batch b (at most max_spans_per_launch spans) on `s`: the plan,
// room in the slabs, the order before, the path's launcher, the mark after.
int ingest_launch(sa_engine *e, const sa_span_batch *b, hipStream_t s) {
  if (b->n == 0) return SA_OK;
  const LaunchPlan pl = plan_launch(e, b->n);
  if (pl.slab_load) {
    if (int rc = make_slab_room(e, pl.slab_load)) return rc;
    e->small.slab_load += pl.slab_load;
  }
  const uint32_t set = e->order.set;
  if (int rc = order_before(e, s, set, 1)) return rc;
  IngestParams P{};
  fill_params(e, b, set, pl, P);
  hipStream_t hs = s;  // the stream the launch's last kernel runs on (expo: the histogram kernels')
  int rc = SA_OK;
  // the latency histograms first, on `s`: the set event mark_after records
  // is behind them on every path (a scatter, an ingest kernel or the
  // histogram kernels follow on `s`, or wait for something that does)
  if ((rc = launch_latency(e, b->n, P, s))) return rc;
  switch (e->path) {
    case Path::Small: rc = launch_small(e, pl.grid, P, s); break;
    case Path::Binned:
    case Path::Dense: rc = launch_binned(e, b->n, P, s); break;
    case Path::Partitioned: rc = launch_partitioned(e, b->n, P, s); break;
    case Path::ExpoSmall:
    case Path::ExpoHbm: rc = launch_expo(e, b, set, pl.grid, P, s, hs); break;
    case Path::Atomic: rc = launch_atomic(e, pl.grid, P, s); break;
  }
  if (rc) return rc;
  // (laboratory build: SPANAGG_NO_SETEV=1 skips the slab-set event -- only
  // valid when every launch uses one stream; it prices the event's cost)
  if ((rc = mark_after(e, hs, set, 1, !lab().no_setev))) return rc;
  e->spans += b->n;
  e->unflushed = true;
  return SA_OK;
}

// Splits a batch at the path's launch limit.
int ingest_on(sa_engine *e, const sa_span_batch *b, hipStream_t s) {
  const uint64_t max_n = max_spans_per_launch(e);
  for (uint64_t off = 0; off < b->n; off += max_n) {
    const uint64_t m = std::min(max_n, b->n - off);
    sa_span_batch sub{b->key_hash + off, b->start_ns + off, b->end_ns + off, b->trace_w0 + off,
                      b->trace_w1 + off, b->meta + off, m};
    if (int rc = ingest_launch(e, &sub, s)) return rc;
  }
  return SA_OK;
}

int check_batch(sa_engine *e, const sa_span_batch *b, bool device) {
  if (!e) return SA_EINVAL;
  if (!b) return fail(e, SA_EINVAL, "null batch");
  if (b->n == 0) return SA_OK;
  const void *cols[5] = {b->key_hash, b->start_ns, b->end_ns, b->trace_w0, b->trace_w1};
  for (const void *c : cols) {
    if (!c) return fail(e, SA_EINVAL, "null batch column");
    if (device && (reinterpret_cast<uintptr_t>(c) & 15))
      return fail(e, SA_EINVAL, "device batch u64 columns must be 16-byte aligned");
  }
  if (!b->meta) return fail(e, SA_EINVAL, "null meta column");
  if (device && (reinterpret_cast<uintptr_t>(b->meta) & 7))
    return fail(e, SA_EINVAL, "device batch meta column must be 8-byte aligned");
  return SA_OK;
}

// true when every column of the batch lies in page-locked host memory
bool batch_pinned(const sa_span_batch *b) {
  const void *cols[6] = {b->key_hash, b->start_ns, b->end_ns, b->trace_w0, b->trace_w1, b->meta};
  for (const void *c : cols) {
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, c) != hipSuccess) {
      (void)hipGetLastError();  // pageable memory: an error the runtime must not keep
      return false;
    }
    if (a.type != hipMemoryTypeHost) return false;
  }
  return true;
}

// m spans of the batch's six columns from `off` into the device slot d (column
// stride ms), asynchronously on the engine stream; ev_b marks the copies' end.
int copy_columns(sa_engine *e, char *d, const sa_span_batch *b, uint64_t off, uint64_t m, uint64_t ms) {
  const uint64_t *src[5] = {b->key_hash + off, b->start_ns + off, b->end_ns + off, b->trace_w0 + off,
                            b->trace_w1 + off};
  for (int c = 0; c < 5; ++c)
    SA_HIP(e, hipMemcpyAsync(d + c * ms * 8, src[c], m * 8, hipMemcpyHostToDevice, e->stream));
  SA_HIP(e, hipMemcpyAsync(d + 5 * ms * 8, b->meta + off, m * 4, hipMemcpyHostToDevice, e->stream));
  SA_HIP(e, hipEventRecord(e->ev_b, e->stream));
  return SA_OK;
}

// Host batches: each chunk is packed into a pinned slot (CPU copy, 44 B/span),
// copied to HBM by DMA and aggregated on the engine stream; the call returns
// once the batch has been copied out of the caller's buffers, so the caller
// builds the next batch while this one is in flight (two slots).
int ingest_host(sa_engine *e, const sa_span_batch *b, bool async) {
  if (int rc = check_batch(e, b, false)) return rc;
  if (b->n == 0) return SA_OK;
  if (int rc = set_dev(e)) return rc;
  // No join: ingest_launch orders each launch itself (slab-set and record-set
  // events), so a binned record set still pending from an earlier call --
  // host or device ingest -- pairs with this call's first launch instead of
  // being aggregated alone.  A pending aggregate that failed earlier is
  // reported here as at every read.
  if (e->binned.sticky_rc) return e->binned.sticky_rc;
  sa_engine::HostStage &h = e->host;
  if (!h.ev_async)
    if (!(h.ev_async = e->res.new_event(hipEventDisableTiming))) return fail(e, SA_EDEVICE, "event creation failed");
  constexpr uint64_t kChunk = sa::kHostChunkSpans;
  constexpr size_t kSlotBytes = kChunk * 44 + 256;
  if (!h.pin[0]) {
    for (int k = 0; k < 2; ++k) {
      if (!(h.pin[k] = static_cast<char *>(e->res.pinned(kSlotBytes))) ||
          dalloc(e, h.dstage[k], kSlotBytes, false))
        return fail(e, SA_ENOMEM, "ingest staging allocation failed");
      if (!(h.pin_ev[k] = e->res.new_event(hipEventDisableTiming))) return fail(e, SA_EDEVICE, "event creation failed");
    }
  }
  const bool pinned = batch_pinned(b);
  // page-locked columns are copied asynchronously: an error return after the
  // first copy still waits for the copies in flight (the caller may reuse or
  // free its columns as soon as the call returns, whatever it returned)
  struct CopyGuard {
    hipStream_t s;
    bool armed;
    ~CopyGuard() {
      if (armed) (void)hipStreamSynchronize(s);
    }
  } guard{e->stream, pinned};
  for (uint64_t off = 0; off < b->n; off += kChunk) {
    const uint64_t m = std::min(kChunk, b->n - off);
    const uint64_t ms = (m + 1) & ~1ULL;  // column stride: u64 columns stay 16-byte aligned
    const int k = h.pin_cur;
    h.pin_cur ^= 1;
    const bool pack = !pinned && m < sa::kHostPageableMin;
    // the packing path rewrites the pinned slot: its last reader (the copy of
    // two chunks back) must be done.  The other paths only reuse the device
    // slot, which stream order protects.
    if (h.pin_used[k] && pack) SA_HIP(e, hipEventSynchronize(h.pin_ev[k]));
    char *d = h.dstage[k];
    if (pack) {
      char *p = h.pin[k];
      const uint64_t *src[5] = {b->key_hash + off, b->start_ns + off, b->end_ns + off, b->trace_w0 + off,
                                b->trace_w1 + off};
      for (int c = 0; c < 5; ++c) std::memcpy(p + c * ms * 8, src[c], m * 8);
      std::memcpy(p + 5 * ms * 8, b->meta + off, m * 4);
      SA_HIP(e, hipMemcpyAsync(d, p, 5 * ms * 8 + m * 4, hipMemcpyHostToDevice, e->stream));
    } else {
      // page-locked columns (sa_host_alloc): DMA straight from them, no
      // packing; the copies are waited for after the last chunk.
      // Large pageable chunks: the runtime's own staging of pageable memory
      // copies faster than one host thread packing the pinned slot.  HIP does
      // not promise that an asynchronous copy from pageable memory has taken
      // the caller's bytes when it returns, so wait for these copies (not for
      // the aggregation) before the caller may reuse or free its columns.
      if (int rc = copy_columns(e, d, b, off, m, ms)) return rc;
      if (!pinned) SA_HIP(e, hipEventSynchronize(e->ev_b));
    }
    const uint64_t *dc = reinterpret_cast<const uint64_t *>(d);
    sa_span_batch sub{dc, dc + ms, dc + 2 * ms, dc + 3 * ms, dc + 4 * ms,
                      reinterpret_cast<const uint32_t *>(d + 5 * ms * 8), m};
    if (int rc = ingest_on(e, &sub, e->stream)) return rc;
    SA_HIP(e, hipEventRecord(h.pin_ev[k], e->stream));
    h.pin_used[k] = true;
  }
  // page-locked columns: every chunk's copies are done (stream order) once
  // the last chunk's are, before the caller may reuse the arrays -- or, for
  // sa_ingest_async, the previous async call's copies (earlier on the stream)
  if (pinned && async) {
    if (h.async_pending) SA_HIP(e, hipEventSynchronize(h.ev_async));
    SA_HIP(e, hipEventRecord(h.ev_async, e->stream));
    h.async_pending = true;
  } else if (pinned) {
    SA_HIP(e, hipEventSynchronize(e->ev_b));
  }
  guard.armed = false;
  return SA_OK;
}

}  // namespace

extern "C" {

int sa_ingest_device(sa_engine *e, const sa_span_batch *b, void *stream) {
  if (int rc = check_batch(e, b, true)) return rc;
  if (int rc = set_dev(e)) return rc;
  // stream-ordered on `stream`: after the engine's earlier work, before the
  // caller's later work on the same stream; launches on other streams may
  // overlap it (see sa_engine::Order)
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  return ingest_on(e, b, s);
}

// k device batches in order on `stream`, as k sa_ingest_device calls would
// ingest them.  Small-table engines (no diagnostics) launch the
// k kernels as one HIP graph: no per-launch dispatch gap between them.  Any
// other engine, a batch that would split, or a slab reduction due inside the
// k launches takes the stream path, one launch after another.
int sa_ingest_device_many(sa_engine *e, const sa_span_batch *bs, uint32_t k, void *stream) {
  if (!e) return SA_EINVAL;
  if (k && !bs) return fail(e, SA_EINVAL, "null batch array");
  for (uint32_t i = 0; i < k; ++i)
    if (int rc = check_batch(e, &bs[i], true)) return rc;
  if (int rc = set_dev(e)) return rc;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  // (SA_OPT_WINDOW_LATENCY: one by one, each launch with its latency kernel)
  bool graph = k > 1 && e->path == Path::Small && !e->dbg && !e->diag() && !e->lat.ring;
  std::vector<LaunchPlan> pl(graph ? k : 0);
  uint64_t load = 0;
  for (uint32_t i = 0; graph && i < k; ++i) {
    graph = bs[i].n != 0 && bs[i].n <= max_spans_per_launch(e);
    if (graph) load += (pl[i] = plan_launch(e, bs[i].n)).slab_load;
  }
  if (graph) {
    if (int rc = make_slab_room(e, load)) return rc;
    graph = load <= kSlabLimit;
  }
  if (!graph) {
    for (uint32_t i = 0; i < k; ++i)
      if (int rc = ingest_on(e, &bs[i], s)) return rc;
    return SA_OK;
  }
  // the ordering ingest_launch gives each launch, once for the k
  const uint32_t first = e->order.set, nsets = e->order.nsets;
  if (int rc = order_before(e, s, first, k)) return rc;
  sa_engine::Small::GraphIngest &g = e->small.gi[e->small.gi_next];
  if (g.launched) SA_HIP(e, hipEventSynchronize(g.done));  // its previous launch is over
  std::vector<IngestParams> P(k);
  std::vector<void *> args(k);
  std::vector<hipKernelNodeParams> np(k);
  for (uint32_t i = 0; i < k; ++i) {
    fill_params(e, &bs[i], (first + i) % nsets, pl[i], P[i]);
    args[i] = &P[i];
    sa::ingest_small_node(pl[i].grid, e->lds_bytes, e->small_kernel, &args[i], &np[i]);
  }
  const bool reuse = g.x && g.nodes.size() == k && g.fn == np[0].func && g.lds == e->lds_bytes &&
                     g.block.x == np[0].blockDim.x;
  if (reuse) {
    for (uint32_t i = 0; i < k; ++i) SA_HIP(e, hipGraphExecKernelNodeSetParams(g.x, g.nodes[i], &np[i]));
  } else {
    if (g.x) (void)hipGraphExecDestroy(g.x);
    if (g.g) (void)hipGraphDestroy(g.g);
    g.x = nullptr;
    g.g = nullptr;
    g.nodes.assign(k, nullptr);
    SA_HIP(e, hipGraphCreate(&g.g, 0));
    for (uint32_t i = 0; i < k; ++i)
      SA_HIP(e, hipGraphAddKernelNode(&g.nodes[i], g.g, i ? &g.nodes[i - 1] : nullptr, i ? 1 : 0, &np[i]));
    SA_HIP(e, hipGraphInstantiate(&g.x, g.g, nullptr, nullptr, 0));
    if (!g.done)
      if (!(g.done = e->res.new_event(hipEventDisableTiming))) return fail(e, SA_EDEVICE, "event creation failed");
    g.fn = np[0].func;
    g.lds = e->lds_bytes;
    g.block = np[0].blockDim;
  }
  if (hipError_t st = hipGraphLaunch(g.x, s); st != hipSuccess)
    return fail(e, SA_EDEVICE, std::string("ingest graph launch: ") + hipGetErrorString(st));
  SA_HIP(e, hipEventRecord(g.done, s));
  g.launched = true;
  e->small.gi_next ^= 1u;
  if (int rc = mark_after(e, s, first, k)) return rc;
  for (uint32_t i = 0; i < k; ++i) e->spans += bs[i].n;
  e->small.slab_load += load;
  e->unflushed = true;
  return SA_OK;
}

int sa_host_alloc(size_t bytes, void **out) {
  if (!out) return SA_EINVAL;
  *out = nullptr;
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    *out = nullptr;
    return SA_ENOMEM;
  }
  return SA_OK;
}

void sa_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}

int sa_ingest(sa_engine *e, const sa_span_batch *b) { return ingest_host(e, b, false); }
int sa_ingest_async(sa_engine *e, const sa_span_batch *b) { return ingest_host(e, b, true); }

int sa_join(sa_engine *e, void *stream) {
  if (!e) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : e->stream;
  if (int rc = bt_aggregate_pending(e)) return rc;
  if (e->binned.sticky_rc) return e->binned.sticky_rc;
  return join_onto(e, s, [&](hipEvent_t ev) -> int {
    SA_HIP(e, hipStreamWaitEvent(s, ev, 0));
    return SA_OK;
  });
}

int sa_sync(sa_engine *e) {
  if (!e) return SA_EINVAL;
  if (int rc = set_dev(e)) return rc;
  if (int rc = join_checked(e)) return rc;
  SA_HIP(e, hipStreamSynchronize(e->stream));
  return SA_OK;
}

}  // extern "C"
