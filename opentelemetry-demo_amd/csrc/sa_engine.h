// sa_engine.h -- internal: struct sa_engine and what the engine's sources
// share.  engine_create.cpp validates, picks the path (sa_path.h) and owns
// creation and destruction; engine_ingest.cpp launches; three files read back:
// engine_read.cpp (flush, reclamation, stats, sa_bind_ids, the probes, one
// window's sketches and the merge hooks), engine_window.cpp (the queries over
// the sketch ring: range, series, top, movers, overlap) and engine_latency.cpp
// (latency, latency movers, SLO burn and latency onset).  One engine owns one
// gfx950 device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "sa_internal.h"
#include "sa_lab.h"
#include "sa_path.h"
#include "sa_query_args.h"
#include "spanagg.h"

// internal to the library: none of this is exported
#pragma GCC visibility push(hidden)

constexpr uint32_t kMaxSlabSets = 4;  // per-workgroup slab sets (small path)

// Everything the engine creates on the device, in creation order.  Each
// maker records what it made and how to release it; sa_destroy releases the
// record in reverse, so a new buffer, event or stream needs no line there.
struct Resources {
  struct Item {
    void *h;
    void (*release)(void *);
  };
  std::vector<Item> items;
  template <class H>  // (h by reference: read only after the call that made it, whatever the argument order)
  H keep(hipError_t st, H &h, void (*release)(void *)) {
    if (st != hipSuccess) return nullptr;
    items.push_back({h, release});
    return h;
  }
  void *device(size_t bytes) {
    void *p = nullptr;
    return keep(hipMalloc(&p, bytes), p, [](void *h) { (void)hipFree(h); });
  }
  void *pinned(size_t bytes) {
    void *p = nullptr;
    return keep(hipHostMalloc(&p, bytes, hipHostMallocDefault), p, [](void *h) { (void)hipHostFree(h); });
  }
  hipEvent_t new_event(unsigned flags) {
    hipEvent_t ev = nullptr;
    return keep(hipEventCreateWithFlags(&ev, flags), ev, [](void *h) { (void)hipEventDestroy((hipEvent_t)h); });
  }
  hipStream_t new_stream(unsigned flags) {
    hipStream_t s = nullptr;
    return keep(hipStreamCreateWithFlags(&s, flags), s, [](void *h) {
      (void)hipStreamSynchronize((hipStream_t)h);
      (void)hipStreamDestroy((hipStream_t)h);
    });
  }
  void release(size_t i) {  // now (hipFree waits for the device), and forget
    items[i].release(items[i].h);
    items.erase(items.begin() + (ptrdiff_t)i);
  }
  void release(void *h) {
    for (size_t i = items.size(); h && i-- > 0;)
      if (items[i].h == h) return release(i);
  }
  void release_all() {
    while (!items.empty()) release(items.size() - 1);
  }
};

// A query's growing device buffer: p holds cap elements (grow, below).
template <class T>
struct DevBuf {
  T *p = nullptr;
  uint64_t cap = 0;
};

struct sa_engine {
  sa_config cfg{};
  sa::Hist hist;  // cfg.bounds points into it
  sa::Path path = sa::Path::Atomic;
  int dev = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev_a = nullptr, ev_b = nullptr;
  // Slab sets ("Launch ordering"): launches alternate
  // between nsets sets of per-workgroup slabs.  ev_set[i]: the end of the last
  // launch that used set i (on set_stream[i]); reads join every set onto the
  // engine stream, and the next launch orders after them through ev_ctl.
  struct Order {
    uint32_t nsets = 1, set = 0;
    hipEvent_t ev_set[kMaxSlabSets] = {}, ev_ctl = nullptr;
    hipStream_t set_stream[kMaxSlabSets] = {};
    bool ctl_dirty = true;
  } order;
  uint32_t log2cap = 0;
  uint64_t cap = 0;
  sa::SmallKernel small_kernel = sa::SmallKernel::Linear;  // Path::Small: the ingest kernel
  int kernel_kind = 0;  // SA_KERNEL_* (spanagg_diag.h): what sa_debug_geometry reports
  uint32_t spl = 4;
  uint32_t G = 0, block = 0, cus = 0;
  size_t lds_bytes = 0;
  unsigned long long *gkeys = nullptr, *gcounts = nullptr, *cms = nullptr, *stats = nullptr, *out_keys = nullptr,
                     *out_rows = nullptr, *scratch = nullptr, *errcnt = nullptr;
  uint64_t *d_seeds = nullptr;
  sa::BinEntry *d_bins = nullptr;  // hist.bins on the device (nullptr: linear thresholds)
  unsigned long long *dbg = nullptr;  // SPANAGG_STAMPS diagnostic timestamps
  uint8_t *hll = nullptr;
  // HLL lower bounds per sub-block of 2^lb_shift registers (IngestParams::hll_lb)
  uint8_t *hll_lb = nullptr;
  uint32_t lb_shift = 0, lb_n = 0, lb_seq = 0;
  unsigned long long *hll_filt = nullptr;  // [kFiltSlots] filtered HLL updates per workgroup slot
  struct Small {
    uint32_t *slab_cnt = nullptr;
    unsigned long long *slab_sum = nullptr;
    uint64_t slab_load = 0;
    // v2: [G][n_windows << log2cap] per-workgroup ERROR counts (the small
    // exponential tables' kernel keeps them too)
    uint32_t *errslab = nullptr;
    // sa_ingest_device_many: two instantiated graphs of K launches, used in
    // turn; one is re-pointed at new batches only after its last launch (done)
    struct GraphIngest {
      hipGraph_t g = nullptr;
      hipGraphExec_t x = nullptr;
      hipEvent_t done = nullptr;
      bool launched = false;
      std::vector<hipGraphNode_t> nodes;
      const void *fn = nullptr;
      dim3 block{};
      size_t lds = 0;
    } gi[2];
    uint32_t gi_next = 0;
  } small;
  // exponential histograms (spanagg_expo.hip).  Path::ExpoSmall: the
  // small-table kernel in EXPO mode (header partials in xslab [G][cap], per-span slots)
  struct Expo {
    sa::XHdr *xslab = nullptr;
    // slab bucket counting of small expo tables (spanagg_expo.hip expo_count_slab_kernel)
    uint32_t xc_ne = 0;
    uint32_t *xc_lcount = nullptr, *xc_slot_of_entry = nullptr, *xcslab = nullptr;
    // the counting kernel's entry selections, double-buffered by launch parity
    // (xc_sel): each launch counts with the selection the previous one made
    // from its counts -- slot_of_entry [2][xc_ne], entry of each slot [2][cap]
    int32_t *xc_ent = nullptr;
    uint32_t xc_sel = 0;
    bool xc_sel_made = false;
    uint32_t *xt_rec = nullptr, *xt_off = nullptr;  // the counting kernel's tail records (ExpoParams::xt_*)
    sa::ExpoHdr *hdr = nullptr;
    int8_t *xscale = nullptr;  // [cap] the slots' scales for the ingest kernel (index records)
    uint32_t *buckets = nullptr, *slot = nullptr;
    uint32_t xidx = 1;  // IngestParams::xidx of index records (laboratory build: SPANAGG_XIDX_OFF)
    uint64_t slot_cap = 0;  // spans per set of slot ([nsets][cap], 8 B each)
    // launch k + 1's ingest kernel runs beside launch k's histogram kernels;
    // its reduce waits for ev_expo, launch k's fold (one owner of the headers)
    hipEvent_t ev_expo = nullptr;
    hipStream_t last = nullptr;
    // laboratory build (SPANAGG_XSTREAM=1): the histogram kernels on an engine
    // stream, after ev_ing[set] on the launch's ingest kernel (slower by A/B)
    hipStream_t xstream = nullptr;
    hipEvent_t ev_ing[kMaxSlabSets] = {};
    unsigned long long *out_keys = nullptr;
    sa::ExpoRow *out_rows = nullptr;
    uint32_t *out_buckets = nullptr;
  } expo;
  // partitioned HBM-table path (lazily allocated on the first launch)
  struct Part {
    ulonglong2 *rec = nullptr;
    uint32_t *fill = nullptr;
  } part;
  // binned-table path (spanagg_binned.hip; DESIGN.md sections 2 and 4): bins of
  // 2^log2sb slots, stored ids m = key * kmul, the spill array base64, lazily
  // allocated record sets
  struct Binned {
    uint32_t log2sb = 0, grid = 0;
    uint64_t kmul = 1, kinv = 1;
    size_t agg_lds = 0;
    // Launch pipeline ("Launch pipeline", "Paired aggregates" in DESIGN.md):
    // scatters on the caller's stream, aggregates on agg_stream, two launches'
    // records per aggregate; a pending set (pend) is aggregated alone before
    // anything reads.  A scatter waits only for the aggregate that last read its set.
    static constexpr int kSets = 4;
    ulonglong2 *rec[kSets] = {};
    uint32_t *cnt[kSets] = {};
    hipStream_t agg_stream = nullptr;
    hipEvent_t ev_scat[kSets] = {}, ev_agg[kSets] = {};
    bool agg_used[kSets] = {};
    uint32_t set = 0;
    int pend = -1;              // the set whose records await the next launch's (or a join)
    int sticky_rc = 0;          // a pending aggregate that failed to launch (join_checked)
    sa::IngestParams pend_P{};  // its launch parameters
    unsigned long long *base64 = nullptr;
    // Path::Dense (spanagg_dense.hip): the same tables and pipeline; gkeys[row
    // of i] is the hash sa_bind_ids bound to index i (kmul = kinv = 1).  `bound`:
    // one bit per index, on the host; bind_buf: sa_bind_ids' device staging.
    std::vector<uint64_t> bound;
    uint64_t n_bound = 0;
    uint64_t *bind_buf = nullptr;
    uint64_t bind_cap = 0;
  } binned;
  size_t hll_slot_bytes = 0, cms_slot_elems = 0;
  // sa_window_range (allocated by its first call): the histogram
  // [n_services][SA_HLL_HIST_BINS], the merged registers (SA_RANGE_REGISTERS
  // only), the summed cells, and the keys with their answers (the two halves of
  // keys); cells_base: a second [d][w], the baseline range's sum (sa_window_movers only)
  struct Range {
    uint32_t *hist = nullptr;
    uint8_t *regs = nullptr;
    unsigned long long *cells = nullptr, *cells_base = nullptr;
    DevBuf<uint64_t> keys;
  } range;
  // sa_window_series (grown by the calls that need more): every output's
  // histogram [n_out][n_services][SA_HLL_HIST_BINS], the windows' row-0 sums
  // [n_windows], the keys and their answers [n_out][n_keys]
  struct Series {
    DevBuf<uint32_t> hist;
    unsigned long long *row0 = nullptr;
    DevBuf<unsigned long long> errors;
    DevBuf<uint64_t> keys;
  } series;
  // sa_window_top (allocated by its first call): the matches as (estimate,
  // key) pairs [cap] -- 16 bytes a table slot -- and the counters, the
  // select's state and the k sorted rows (sa::TopCtl, 65 KiB whatever the table)
  struct Top {
    ulonglong2 *cand = nullptr;
    sa::TopCtl *ctl = nullptr;
  } top;
  // sa_window_movers (allocated by its first call) works in sa_window_top's
  // scratch -- calls are serialised -- and leaves the baseline's error_spans
  // and the rows' estimates here (sa::MoversOut, 64 KiB)
  struct Movers {
    sa::MoversOut *out = nullptr;
  } movers;
  // sa_window_error_onset (allocated by its first call) works in
  // sa_window_top's scratch too, and leaves the eligible keys' count and the
  // rows' splits here (sa::ErrOnsetOut, 96 KiB)
  struct ErrOnset {
    sa::ErrOnsetOut *out = nullptr;
  } err_onset;
  // sa_window_overlap (allocated by its first call, for min(n_services,
  // SA_OVERLAP_MAX_SERVICES) = cap services): the selected ids [cap], their
  // merged registers [cap][2^p] and histograms [cap][SA_HLL_HIST_BINS], and
  // the pairs' histograms [cap (cap - 1) / 2][SA_HLL_HIST_BINS]
  struct Overlap {
    uint32_t *map = nullptr, *hist = nullptr, *pair_hist = nullptr;
    uint8_t *regs = nullptr;
  } overlap;
  // SA_OPT_WINDOW_LATENCY (spanagg_latency.hip; nullptr without the option):
  // ring [n_windows][n_services][SA_LAT_BINS] u64, the ring slots the ingest
  // kernel holds in LDS (0: the HBM form) and its largest grid; and the scratch
  // of the four queries over it, one buffer a role, grown (DevBuf) or allocated
  // (lazy) by the calls that need it.  The queries share them because calls on
  // an engine are serialised, and a group query runs export -> reduce -> finish
  // on one engine without another query between: what a stage leaves (the
  // onset's thr from its pairs stage to its finish) is still there, and a
  // finish asks for no more than its export did, so nothing it needs is regrown.
  // The select works in sa_window_top's control block.
  struct Latency {
    unsigned long long *ring = nullptr;
    uint32_t k_slots = 0, grid_max = 0;
    DevBuf<uint32_t> sel;  // a selection's service ids (latency, SLO)
    DevBuf<uint8_t> thr;   // threshold bins, one an id (SLO: the selection's; onset: every service's)
    DevBuf<unsigned long long> pairs;    // the engine's own (total, slow) pairs [ids][n_cov][2] (SLO, onset, the probe)
    DevBuf<unsigned long long> prefix;   // the SLO's prefix sums [n_sel][n_cov + 1][2]
    DevBuf<unsigned long long> slo_out;  // the SLO's answers: total, slow, alert, burning
    unsigned long long *range_sums = nullptr;  // the engine's own [2][n_services][SA_LAT_BINS] (movers; onset: the first)
    unsigned long long *counts = nullptr;      // the movers' [2][n_services]
    // the ranking scans' candidates and the onset's best splits, one an id (the probe's ids need not be the
    // engine's) -- cand its own: sa_window_top's holds a table's slots, which can be fewer
    DevBuf<ulonglong2> cand;
    DevBuf<sa::OnsetRow> rec;
    union Ranked {  // the ranked rows: a 16-byte head, then kTopSel rows
      sa::LatMovOut mov;
      sa::OnsetOut onset;
    } *ranked = nullptr;
    // sa_window_latency's own: one tile of sliding sums [rows][SA_LAT_BINS], every row's count and quantile bins
    DevBuf<unsigned long long> sums, count;
    DevBuf<uint8_t> q_bin;
  } lat;
  // sa_ingest: two pinned host slots and their HBM copies; a slot is refilled
  // once its event (H2D copy + aggregation of the previous use) has passed
  struct HostStage {
    char *pin[2] = {nullptr, nullptr}, *dstage[2] = {nullptr, nullptr};
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    bool pin_used[2] = {false, false};
    // sa_ingest_async: the event after the last async call's copies (its
    // columns are the caller's until that event completes)
    hipEvent_t ev_async = nullptr;
    bool async_pending = false;
    int pin_cur = 0;
  } host;
  uint64_t win_base = 0, spans = 0, dropped_seen = 0;
  bool unflushed = false;   // spans ingested since the RED counters were last reset
  uint64_t reclaims = 0;    // key-table reclamations (sa_reclaim_keys)
  Resources res;
  std::string err;

  bool dense() const { return path == sa::Path::Dense; }
  bool diag() const { return cfg.flags != 0; }  // SA_DIAG_* flags (laboratory build; the product's sa_create refuses them)
};

inline int fail(sa_engine *e, int code, const std::string &msg) {
  if (e) e->err = msg;
  return code;
}

#define SA_HIP(e, call)                                                                   \
  do {                                                                                    \
    hipError_t _st = (call);                                                              \
    if (_st != hipSuccess)                                                                \
      return fail((e), SA_EDEVICE, std::string(#call) + ": " + hipGetErrorString(_st));  \
  } while (0)

inline int set_dev(sa_engine *e) {
  SA_HIP(e, hipSetDevice(e->dev));
  return SA_OK;
}

// Device memory through the engine's owner: SA_ENOMEM with `what` when the
// allocation fails, SA_EDEVICE when zeroing does.
template <class T>
int dalloc(sa_engine *e, T *&p, size_t count, bool zeroed, const char *what = "hipMalloc failed") {
  p = static_cast<T *>(e->res.device((count ? count : 1) * sizeof(T)));
  if (!p) return fail(e, SA_ENOMEM, what);
  if (zeroed && hipMemset(p, 0, count * sizeof(T)) != hipSuccess) return fail(e, SA_EDEVICE, "hipMemset failed");
  return SA_OK;
}
template <class T>
void dfree(sa_engine *e, T *&p) {
  e->res.release(p);
  p = nullptr;
}
// A query's scratch, allocated by the first call that needs it.
template <class T>
int lazy(sa_engine *e, T *&p, size_t count, const char *what) {
  return p ? SA_OK : dalloc(e, p, count, false, what);
}
// p (holding cap elements) grown to at least `want`, its contents dropped.
template <class T>
int grow(sa_engine *e, T *&p, uint64_t &cap, uint64_t want, const char *what) {
  if (want <= cap) return SA_OK;
  dfree(e, p);  // (hipFree waits for the device)
  cap = 0;
  if (int rc = dalloc(e, p, want, false, what)) return rc;
  cap = want;
  return SA_OK;
}
template <class T>
int grow(sa_engine *e, DevBuf<T> &b, uint64_t want, const char *what) {
  return grow(e, b.p, b.cap, want, what);
}
// The call's one wait on `s` -- also after a failure st of what was queued:
// copies may be in flight -- and SA_EDEVICE "<query>: <error>" when either failed.
inline int wait_or_fail(sa_engine *e, hipError_t st, hipStream_t s, const char *query) {
  const hipError_t waited = hipStreamSynchronize(s);
  if (st == hipSuccess && waited == hipSuccess) return SA_OK;
  return fail(e, SA_EDEVICE, std::string(query) + ": " + hipGetErrorString(st != hipSuccess ? st : waited));
}

// An argument rule's verdict (sa_query_args.h) as the call's: "<query>: <what is wrong>"
inline int bad_args(sa_engine *e, int code, const char *query, const char *bad) {
  return fail(e, code, std::string(query) + ": " + bad);
}
// sa_args::span on the engine's ring: SA_ERANGE unless every window the
// outputs first..last cover, `width` windows each, is resident
inline int check_span(sa_engine *e, const char *query, uint64_t first, uint64_t last, uint32_t width = 1) {
  if (const char *bad = sa_args::span(first, last, width, e->win_base, e->cfg.n_windows))
    return bad_args(e, SA_ERANGE, query, bad);
  return SA_OK;
}

// engine_ingest.cpp
// Orders the engine stream after every outstanding launch (each set's last
// user); join_checked: SA_EDEVICE (with e->err) when a pending aggregate could
// not be launched -- for the calls that read or reorder.
void join_sets(sa_engine *e);
int join_checked(sa_engine *e);
int reduce_slabs(sa_engine *e, hipStream_t s);
sa::ExpoParams expo_params(sa_engine *e, const sa_span_batch *b, uint32_t set = 0);
uint32_t bt_region_for(const sa_engine *e, uint64_t wg_chunk);

// engine_read.cpp
// Every read starts here: the engine's device, and every launch in flight
// joined onto the engine stream (a pending aggregate that failed is returned).
int begin_read(sa_engine *e);
// A caller's stream `s` takes over from the engine stream (ev_a), and hands
// back: later engine work orders after what the caller's stream did (ev_b).
int hop_to(sa_engine *e, hipStream_t s);
int hop_back(sa_engine *e, hipStream_t s);
// Derive the count-min cells of window slot ws from its exact per-slot error
// counts (see sketch_post in sa_device.h).
int fold_errslab(sa_engine *e, uint64_t ws, hipStream_t s);

// engine_window.cpp
// After a ranked launch (st: what it returned) on `s`, not waited for: sa::TopCtl's
// head and its first k selected pairs, and the out block's 16-byte head with
// its first k rows of row_bytes each (sa::MoversOut, LatMovOut, OnsetOut) into `block`.
hipError_t copy_ranked(hipError_t st, const sa::TopCtl *ctl, uint32_t k, unsigned long long head[4], ulonglong2 *sel,
                       const void *d_out, size_t row_bytes, void *block, hipStream_t s);

#pragma GCC visibility pop
