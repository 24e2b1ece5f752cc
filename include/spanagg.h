/*
 * spanagg.h -- C-ABI of libspanagg, the MI355X (gfx950) span-aggregation engine.
 *
 * Drop-in replacement for the per-span work of the otel-collector `spanmetrics`
 * connector that the reference demo wires into its traces pipeline
 * (/root/reference/src/otel-collector/otelcol-config.yml:115-116 declares it,
 * :118-127 makes it an exporter of `traces` and a receiver of `metrics`).
 * The connector itself is Go ([UPSTREAM] opentelemetry-collector-contrib
 * connector/spanmetricsconnector v0.125.0, image tag /root/reference/.env:14);
 * its source is not vendored, so the upstream entry points are cited by name.
 *
 *   upstream (Go)                                   replaced by
 *   ----------------------------------------------  -------------------------------
 *   createDefaultConfig / Config                    sa_config + sa_config_default
 *   createTracesToMetricsConnector, Start           sa_create
 *   ConsumeTraces -> aggregateMetrics (per span)    sa_ingest / sa_ingest_async / sa_ingest_device
 *   exportMetrics -> buildMetrics + resetState      sa_flush (+ host-side encoding)
 *   Shutdown                                        sa_destroy
 *   (new) per-service HLL + error count-min         sa_window_read / sa_window_advance
 *   (new) the same over a span of windows           sa_window_range (merged on the device)
 *   (new) every trailing span of a window series    sa_window_series (one pass over the ring)
 *   (new) heavy hitters over a span of windows      sa_window_top (key table scanned on the device)
 *   (new) traces shared by pairs of services        sa_window_overlap (pairwise register maxima on the device)
 *   (new) series whose ERROR rate changed most      sa_window_movers (key table against two ranges' cells on the device)
 *   (new) when each series began to fail            sa_window_error_onset (every split of a range per resident key, one walk over the ring's cells on the device)
 *   (new) duration quantiles per service and window sa_window_latency (log-linear histograms in the ring, SA_OPT_WINDOW_LATENCY)
 *   (new) services whose latency shifted most       sa_window_latency_movers (two ranges' histograms summed, scored and selected on the device)
 *   (new) latency SLO burn over sliding widths      sa_window_slo (rows cut to (total, slow) pairs at a threshold, prefix sums on the device)
 *   (new) when each service's latency shifted       sa_window_latency_onset (the pairs' change point per service, a 128-bit CUSUM on the device)
 *
 * Boundary rules (mirroring the connector's contracts):
 *  - Ownership: batches are borrowed for the duration of the call (page-locked
 *    columns passed to sa_ingest_async: until the next sa_ingest_async or
 *    sa_sync returns); results are owned by the library and released with
 *    sa_red_result_free / sa_sketch_result_free.
 *  - Errors: every call returns an sa_status (0 ok, <0 error); nothing throws
 *    or aborts across the ABI; sa_last_error() gives the message.
 *  - Threading: one engine is single-producer (the connector serialises
 *    ConsumeTraces and the export ticker on one mutex); callers serialise.
 *  - No torch / HIP types appear in signatures; device pointers and streams
 *    are passed as plain pointers.
 *
 * SoA v1 span batch (44 algorithmic bytes per span, one column per array):
 *   key_hash  u64  series id: hash of (resource identity, NUL-joined metric key);
 *                  computed by the host; 0 is reserved (counted as invalid)
 *   start_ns  u64  span.start_time_unix_nano
 *   end_ns    u64  span.end_time_unix_nano
 *   trace_w0  u64  trace_id bytes 0..7 read little-endian (memcpy of the wire bytes)
 *   trace_w1  u64  trace_id bytes 8..15 read little-endian
 *   meta      u32  bits 0-15 service_id, 16-18 span.kind, 19-20 status.code
 */
#ifndef SPANAGG_H
#define SPANAGG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SA_ABI_VERSION 4
#define SA_MAX_BOUNDS 62

typedef enum {
    SA_OK = 0,
    SA_EINVAL = -1,   /* bad argument / config */
    SA_ENOMEM = -2,   /* host or device allocation failed */
    SA_EDEVICE = -3,  /* HIP runtime error or no usable gfx950 device */
    SA_EFULL = -4,    /* key table full: spans were dropped (see stats) */
    SA_ERANGE = -5,   /* window id outside the resident ring */
    SA_ESTATE = -6    /* call not valid in the engine's current state */
} sa_status;

typedef enum { SA_UNIT_MS = 0, SA_UNIT_S = 1 } sa_unit;

/* Test and profiling entry points (probes of single kernel stages, per-
 * workgroup timestamps) are not connector operations: they are declared in
 * spanagg_diag.h, which this header does not include.
 *
 * Diagnostic ablations (sa_config.flags), used only to attribute kernel time.
 * Only the laboratory build of the library accepts them (`make -C
 * opentelemetry-demo_amd ab` -> libspanagg_ab.so, used by tools/); the
 * product library returns SA_EINVAL for any flags != 0. */
#define SA_DIAG_NO_RED 1u     /* skip key lookup + counter updates */
#define SA_DIAG_NO_HLL 2u     /* skip HLL hashing + register updates */
#define SA_DIAG_NO_CMS 4u     /* skip count-min updates */
#define SA_DIAG_NO_FLUSH 8u   /* skip the LDS -> slab flush */
#define SA_DIAG_L2_INPUT 16u  /* every workgroup re-reads the batch's first 4 tiles
                                 (cache-resident input: prices the HBM stream) */

/* Path options (sa_config.options): each selects another kernel path (or
 * merge transport) that computes the SAME results -- the parity tests compare
 * the paths through them.  0 (the default) lets the engine pick by geometry. */
#define SA_OPT_NO_HLL_FILTER (1u << 0) /* every span gathers its HLL register (no lower-bound filter) */
#define SA_OPT_PARTITIONED   (1u << 1) /* large tables: the partitioned path instead of the binned one */
#define SA_OPT_ATOMIC_TABLE  (1u << 2) /* large tables: per-span HBM CAS + atomics (no partition) */
#define SA_OPT_EXPO_HBM      (1u << 3) /* exponential histograms on the HBM-table kernels at any size */
#define SA_OPT_EXPO_CACHED   (1u << 4) /* small exponential tables: the cached-probe counting kernel */
#define SA_OPT_IDENTITY_IDS  (1u << 5) /* binned table: stored id = series id (no random multiplier) */
#define SA_OPT_STAMPS        (1u << 6) /* per-workgroup timestamps for sa_debug_stamps */
#define SA_OPT_GROUP_COPY    (1u << 7) /* sa_group_create: merge through device copies, never RCCL */
#define SA_OPT_GROUP_RCCL    (1u << 8) /* sa_group_create: RCCL even for a group of one */
/* Dense series indices (large explicit-bucket tables; spanagg_dense.hip): the
 * host resolves each span's series in its own dictionary and the key_hash
 * column of EVERY ingest call (host, async, device, device_many) carries a
 * dense index i instead of the hash.  Index 0 stays "no series" (zero_key);
 * 1 <= i < table_capacity is valid; a span with i >= table_capacity is
 * counted in dropped_table_full (the next flush returns SA_EFULL), still
 * updates its HLL register and adds nothing to the count-min.  sa_bind_ids
 * declares which hash an index stands for; results (flush rows, count-min
 * cells, HLL) equal the default engine's on the same spans with the real
 * hashes.  Spans on an index that was never bound are added to
 * dropped_table_full by the time sa_flush returns (SA_EFULL): no row, no
 * count-min cell.  table_capacity: the next power of two >= 1.25 x
 * key_capacity, at least 2^19.  sa_create returns SA_EINVAL with
 * exp_max_size != 0, more than 17 buckets, n_windows > 1024, bounds the
 * bucket bin table cannot hold, SA_OPT_PARTITIONED / ATOMIC_TABLE / EXPO_HBM /
 * EXPO_CACHED, or a table above 2^22 slots; sa_group_create returns SA_EINVAL
 * (groups merge by hash).  sa_gather_dense and sa_reclaim_keys return
 * SA_ESTATE (no hash -> slot map on the device; nothing is ever full, flush
 * never reclaims); sa_stats.n_keys is the number of bound indices. */
#define SA_OPT_DENSE_IDS     (1u << 9)
/* Latency histograms over the window ring (spanagg_latency.hip): the engine
 * also keeps, per resident window and service, a histogram of span durations
 * in SA_LAT_BINS log-linear bins, read by sa_window_latency.  It combines with
 * every other option and runs beside every ingest path: one more streaming
 * kernel per launch, which reads start_ns, end_ns and meta (20 bytes a span)
 * and no key.  The ring holds n_windows * n_services * SA_LAT_BINS u64:
 * sa_create returns SA_EINVAL when n_windows * n_services > 2^18 (512 MiB)
 * and SA_ENOMEM when the allocation fails.  With the option
 * sa_ingest_device_many takes the one-by-one path (no graph).  Without it
 * nothing is allocated and nothing more is launched. */
#define SA_OPT_WINDOW_LATENCY (1u << 10)
#define SA_OPT_ALL           0x7FFu

typedef struct {
    /* histogram.explicit.buckets (sorted ascending, finite) and histogram.unit */
    const double *bounds;
    uint32_t n_bounds;
    uint32_t unit;          /* sa_unit */
    /* build-owned sketches */
    uint32_t hll_p;         /* HLL precision, 4..18 (default 14) */
    uint32_t cms_d;         /* count-min rows, 1..8 (default 4) */
    uint32_t cms_w;         /* count-min columns, power of two (default 2048) */
    uint64_t window_ns;     /* sketch window length (default 10 s; < 2^56 ns) */
    uint32_t n_windows;     /* resident window ring, power of two (default 8) */
    uint32_t n_services;    /* service ids 0..n_services-1 get sketches */
    uint64_t key_capacity;  /* expected distinct series; table = next pow2 >= 1.25x */
    int32_t device;         /* HIP device ordinal (one engine per GPU / rank) */
    uint32_t flags;         /* 0 for production; SA_DIAG_* bits are profiling-only
                               ablations that skip work and make results WRONG
                               (laboratory build only) */
    /* histogram.exponential.max_size: 0 = explicit buckets (the default);
     * 2..4096 = exponential histograms (bounds unused; read with sa_flush_exp) */
    uint32_t exp_max_size;
    uint32_t options;       /* SA_OPT_* path options (0 = the engine's choice) */
} sa_config;

typedef struct {
    const uint64_t *key_hash, *start_ns, *end_ns, *trace_w0, *trace_w1;
    const uint32_t *meta;
    uint64_t n;
} sa_span_batch;

/* Delta RED state since the previous sa_flush, one row per series with any
 * span, sorted by key_hash ascending. */
typedef struct {
    uint64_t n_series;
    uint32_t n_buckets;            /* n_bounds + 1 */
    const uint64_t *key_hash;      /* [n_series] */
    const uint64_t *bucket_counts; /* [n_series][n_buckets] */
    const uint64_t *calls;         /* [n_series] == sum of bucket_counts (A8) */
    const uint64_t *sum_ns;        /* [n_series] exact sum of durations in ns */
    const double *sum;             /* [n_series] sum_ns / unit divisor (ms or s) */
} sa_red_result;

/* Exponential histograms (sa_config.exp_max_size > 0): the delta since the
 * previous sa_flush_exp, one row per series with any span, sorted by
 * key_hash.  Each row is go-expohisto's Histogram[float64] of the series'
 * durations (float64(end-start)/unit): positive bucket i at `scale` counts
 * values in (2^(i/2^scale), 2^((i+1)/2^scale)]; bucket_counts[r][j] is bucket
 * offset[r] + j for j < n_buckets[r]. */
typedef struct {
    uint64_t n_series;
    uint32_t max_size;             /* row stride of bucket_counts */
    uint32_t unit;                 /* sa_unit of sum/min/max */
    const uint64_t *key_hash;      /* [n_series] */
    const uint64_t *count;         /* [n_series] spans (== calls) */
    const uint64_t *zero_count;    /* [n_series] zero durations */
    const uint64_t *sum_ns;        /* [n_series] exact */
    const double *sum, *min, *max; /* [n_series] in the unit */
    const int32_t *scale, *offset; /* [n_series] */
    const uint32_t *n_buckets;     /* [n_series] */
    const uint64_t *bucket_counts; /* [n_series][max_size] */
} sa_exp_result;

typedef struct {
    uint64_t window_id;
    uint32_t n_services, hll_p;
    const uint8_t *hll;            /* [n_services][2^hll_p] registers */
    uint32_t cms_d, cms_w;
    const uint32_t *cms;           /* [cms_d][cms_w], saturating u32 */
} sa_sketch_result;

typedef struct {
    uint64_t spans;                /* spans accepted by sa_ingest* */
    uint64_t zero_key;             /* spans with key_hash == 0 (no RED update) */
    uint64_t invalid_service;      /* service_id >= n_services (no sketch update) */
    uint64_t window_out_of_range;  /* window outside the resident ring (no sketch update) */
    uint64_t dropped_table_full;   /* spans lost because the key table was full */
    uint64_t n_keys;               /* distinct series resident in the key table */
    uint64_t table_capacity;
    uint64_t window_base;          /* oldest resident window id */
    uint32_t small_table;          /* 1 = LDS-mirrored table path, 0 = HBM path */
    uint32_t pad;
    /* spans whose HLL update was skipped without reading their register: rho
     * at or below the lower bound of the register's sub-block, so it could not
     * raise it (the small-table and binned kernels; 0 on the other paths).
     * Diagnostic: shows how much of a window runs on the filtered path. */
    uint64_t hll_filtered;
} sa_stats;

typedef struct sa_engine sa_engine;

/* createDefaultConfig: default buckets {2,4,6,8,10,50,100,200,400,800,1000,1400,
 * 2000,5000,10000,15000} ms, HLL p=14, CMS 4x2048, 10 s windows, 8-window ring. */
void sa_config_default(sa_config *cfg);
int sa_abi_version(void);

int sa_create(const sa_config *cfg, sa_engine **out);
void sa_destroy(sa_engine *e);
const char *sa_last_error(const sa_engine *e);

/* Host-memory batch: packed into one of two pinned staging slots (chunks of
 * 2^18 spans or more: copied from the caller's pageable columns by the HIP
 * runtime, and waited for), copied to HBM and aggregated on the engine
 * stream.  Returns once the batch has been copied out of the caller's buffers
 * (they may be reused or freed at once); the
 * aggregation completes asynchronously -- every read (sa_flush*, sa_window_*,
 * sa_get_stats) and sa_sync wait for it, and a device error surfaces there. */
int sa_ingest(sa_engine *e, const sa_span_batch *batch);
/* sa_ingest for a host that alternates two page-locked column buffers (the
 * Node host's columnizer): when every column lies in sa_host_alloc memory the
 * DMA reads them after the call returns, and the call returns once the
 * columns of this engine's previous sa_ingest_async call have been read -- so
 * the caller may refill the other buffer while this one is copied, and must
 * leave this one alone until its next sa_ingest_async (or sa_sync /
 * sa_destroy) returns.  Any other columns, and any error return: as
 * sa_ingest (read before the call returns). */
int sa_ingest_async(sa_engine *e, const sa_span_batch *batch);
/* Page-locked host memory for batch columns a host builds itself (the Node
 * host's columnizer does): sa_ingest / sa_group_ingest copy columns that all
 * lie in such memory to HBM by DMA straight from the caller's arrays, with no
 * staging copy on the calling thread.  SA_ENOMEM when no GPU runtime can pin
 * memory (the caller then uses ordinary memory, which sa_ingest stages). */
int sa_host_alloc(size_t bytes, void **out);
void sa_host_free(void *p);
/* Device-resident batch (pointers into HBM of this engine's device).
 * `stream` is a hipStream_t (NULL = the engine's own stream). Asynchronous:
 * the batch must stay valid until the stream reaches this point. Ordered
 * after the engine's earlier non-ingest work (flush, window calls) and
 * before the caller's later work on `stream`; ingests on different streams
 * may run concurrently on the device (the engine orders them only where they
 * share state), which is how consecutive batches overlap. */
int sa_ingest_device(sa_engine *e, const sa_span_batch *batch, void *stream);
/* k device batches in order on `stream`: the same result as k
 * sa_ingest_device calls on it (same ordering rules, every batch valid until
 * the stream reaches the end of the k).  Small-table engines launch the k
 * ingests as one HIP graph, so consecutive launches carry no per-launch
 * dispatch gap; other engines (binned, exponential, laboratory options) and
 * batches that would need a split take the one-by-one path, and so does every
 * engine with SA_OPT_WINDOW_LATENCY.  Unlike
 * sa_ingest_device, the graph path can block the host: the engine keeps two
 * instantiated graphs and, before it re-points one at new batches, waits
 * (hipEventSynchronize) until that graph's previous launch -- the one of two
 * graph calls earlier -- has finished on the device.  Do not call it while
 * holding a lock that `stream`'s pending work needs, nor when `stream` waits
 * on host work queued after this call.  Replaces a loop
 * of ConsumeTraces calls over the batches a receiver queued (the connector's
 * aggregateMetrics per request, connector.go [UPSTREAM]). */
int sa_ingest_device_many(sa_engine *e, const sa_span_batch *batches, uint32_t k, void *stream);
/* Orders `stream` (NULL = the engine's stream) after every launch the engine
 * has enqueued so far, including work it runs on its own streams: the
 * high-cardinality (binned) path aggregates launch k on an engine stream
 * while launch k + 1 reads its batch, so the caller's stream passes an
 * ingest once the batch is consumed, not once it is aggregated.  Engine reads
 * (sa_flush*, sa_window_*, sa_get_stats) and sa_sync join by themselves; a
 * caller timing the aggregation with events on its own stream joins first. */
int sa_join(sa_engine *e, void *stream);
int sa_sync(sa_engine *e);

/* exportMetrics: delta since the last flush, then the engine's RED counters are
 * reset. Keys stay resident as a cache of the series seen, until more than half
 * the table is taken (35 % for the binned table of large key capacities): then
 * the flush empties it (sa_reclaim_keys), so series
 * that churn (new resources after evictions or restarts, delta purges) do not
 * fill it for good. Returns SA_EFULL (with the result still filled) if spans
 * were dropped since the previous flush: more distinct series within one flush
 * interval than key_capacity. */
int sa_flush(sa_engine *e, sa_red_result **out);
void sa_red_result_free(sa_red_result *r);
/* Key-table reclamation (what every flush does when the table is more than
 * half full, binned tables 35 %; force != 0: empty it now).  Only between a flush (or a resetting
 * sa_gather_dense) and the next ingest: SA_ESTATE otherwise.  Results do not
 * change: every row is zero then, and a series' next span re-inserts its key.
 * Replaces nothing in the reference (upstream keys live in a Go LRU map,
 * spanmetrics connector.go `resourceMetrics` / `dimensionsCache`). */
int sa_reclaim_keys(sa_engine *e, int force);
/* exportMetrics of an exponential-histogram engine (sa_flush returns
 * SA_ESTATE there, and sa_flush_exp does on an explicit-bucket engine). */
int sa_flush_exp(sa_engine *e, sa_exp_result **out);
void sa_exp_result_free(sa_exp_result *r);
/* Sketches of one resident window (not cleared). */
int sa_window_read(sa_engine *e, uint64_t window_id, sa_sketch_result **out);
/* Retire every window < new_base (clears their ring slots); spans whose window
 * is below the base or >= base + n_windows are counted in window_out_of_range. */
int sa_window_advance(sa_engine *e, uint64_t new_base);
void sa_sketch_result_free(sa_sketch_result *r);

/* ---- range queries over the window ring ----
 * The sketches of the resident windows first..last (inclusive) merged on the
 * device: HLL registers max-merged, count-min cells summed, point queries for
 * a list of series.  Only the answers cross the bus: without flags a call
 * returns n_services x SA_HLL_HIST_BINS histogram words, the estimates and
 * n_keys counts, whatever the ring holds (one sa_window_read per window copies
 * n_services x 2^hll_p bytes each). */
#define SA_HLL_HIST_BINS 64          /* register values 0 .. 65 - p <= 61 */
#define SA_RANGE_REGISTERS 1u        /* also return the merged registers */
#define SA_RANGE_CELLS     2u        /* also return the summed cells */

typedef struct {
    uint64_t first_window, last_window;      /* inclusive */
    uint32_t n_services, hll_p;
    const uint32_t *hll_hist;  /* [n_services][SA_HLL_HIST_BINS]: registers of the max-merged
                                  array holding value v; every row sums to 2^hll_p */
    const double *distinct;    /* [n_services] sa_hll_estimate_hist(row, hll_p) */
    const uint8_t *hll;        /* [n_services][2^hll_p] merged registers; NULL without SA_RANGE_REGISTERS */
    uint32_t cms_d, cms_w;
    const uint64_t *cms;       /* [cms_d][cms_w] cells summed over the windows, unsaturated;
                                  NULL without SA_RANGE_CELLS */
    uint64_t n_keys;
    const uint64_t *errors;    /* [n_keys] min over rows of the summed cell of keys[i]: the merged
                                  sketch's estimate, an upper bound on the key's ERROR spans */
} sa_range_result;

/* Ordering and waiting as sa_window_read: joins every launch in flight, runs
 * on the engine stream, waits, clears nothing (two calls give equal results).
 * SA_ERANGE when first > last or a window of the range is not resident;
 * SA_EINVAL for a null `out`, n_keys != 0 with null `keys`, unknown flag bits.
 * `keys`: a host array of series hashes borrowed for the call -- hashes also
 * on an SA_OPT_DENSE_IDS engine (the count-min is addressed by the bound
 * hash); key 0 is allowed.  Works on every ingest path.  Free the result with
 * sa_range_result_free. */
int sa_window_range(sa_engine *e, uint64_t first, uint64_t last, const uint64_t *keys,
                    uint64_t n_keys, uint32_t flags, sa_range_result **out);
void sa_range_result_free(sa_range_result *r);

/* ---- sliding series over the window ring ----
 * A detector's time series in one call: for every window t = first..last the
 * answers of sa_window_range over the trailing span t-width+1 .. t ("the last
 * 5 minutes, evaluated every 10 s").  The ring is read a constant number of
 * times whatever the width, and only the answers cross the bus. */
typedef struct {
    uint64_t first_window, last_window;  /* outputs t = first..last, inclusive */
    uint32_t width, n_out;               /* output t covers windows t-width+1 .. t; n_out = last-first+1 */
    uint32_t n_services, hll_p;
    const uint32_t *hll_hist;    /* [n_out][n_services][SA_HLL_HIST_BINS], every row sums to 2^hll_p */
    const double   *distinct;    /* [n_out][n_services] sa_hll_estimate_hist(row, hll_p) */
    const uint64_t *error_spans; /* [n_out] sum of count-min row 0 over the covered windows:
                                    the ERROR spans the sketches counted there, exact */
    uint64_t n_keys;
    const uint64_t *errors;      /* [n_out][n_keys] point query on the covered windows' summed cells */
} sa_series_result;

/* Row t is bit for bit what sa_window_range(e, t-width+1, t, keys, n_keys, 0, ..)
 * returns in hll_hist, distinct and errors.  Ordering and waiting as
 * sa_window_range: joins every launch in flight, runs on the engine stream,
 * waits, clears nothing (two calls give equal bits); works on every ingest
 * path; `keys` are hashes, also on an SA_OPT_DENSE_IDS engine, and key 0 is
 * allowed.  SA_ERANGE when first > last, width == 0, width > n_windows,
 * first + 1 < width, or first-width+1 or last is not resident; SA_EINVAL for a
 * null `out`, n_keys != 0 with null `keys`, or flags != 0 (reserved);
 * SA_ENOMEM when the result or the device scratch cannot be allocated.  The
 * engine stays usable after any error.  Free the result with
 * sa_series_result_free.
 * There is no group entry point: histograms are not additive over members
 * (the maximum is taken register by register first), so a group series would
 * have to all-reduce every window's registers -- the traffic this call exists
 * to avoid.  A group's caller loops sa_group_window_range. */
int sa_window_series(sa_engine *e, uint64_t first, uint64_t last, uint32_t width,
                     const uint64_t *keys, uint64_t n_keys, uint32_t flags, sa_series_result **out);
void sa_series_result_free(sa_series_result *r);

/* ---- heavy hitters over the window ring ----
 * "Which series fail most over these windows": the engine's own key table is
 * the candidate list, so the caller sends no keys and gets k rows back. */
#define SA_TOP_MAX_K 4096u
typedef struct {
    uint64_t first_window, last_window;   /* inclusive */
    uint32_t k, n;                        /* asked for; returned (n <= k) */
    uint64_t n_resident;                  /* series in the key table when the call ran: the candidates */
    uint64_t n_matched;                   /* candidates with estimate >= min_count */
    uint64_t error_spans;                 /* sum of row 0 of the summed cells: ERROR spans counted in the range, exact */
    const uint64_t *key_hash;             /* [n] */
    const uint64_t *errors;               /* [n] */
} sa_top_result;

/* Candidates: every non-zero key resident in the key table when the call
 * runs -- the series seen since the last reclaim, on every ingest path.  On an
 * SA_OPT_DENSE_IDS engine key_hash is the bound hash, and unbound indices are
 * not candidates.  Key 0 is never a candidate; spans that got no slot (table
 * full) are never candidates, although their ERROR spans are in the cells and
 * in error_spans.  A reclaim (sa_reclaim_keys, or the one a flush does once
 * the table is more than half taken) empties the candidates while the cells
 * stay: a caller that must not lose them asks before the flush that reclaims.
 * Estimate: errors[i] is bit for bit what sa_window_range(e, first, last,
 * &key_hash[i], 1, 0, ..) returns -- the minimum over the rows of the cells
 * summed in u64 over first..last.
 * Order: the n_matched candidates with an estimate >= max(min_count, 1),
 * sorted by estimate descending, then key_hash ascending (sketch.heavy_hitters'
 * order; a total order, so ties do not show); the first n = min(k, n_matched)
 * of them are returned, in that order.
 * Ordering and waiting as sa_window_range: joins every launch in flight, runs
 * on the engine stream, waits, clears nothing (two calls give equal bits).
 * SA_EINVAL for a null `out`, k == 0, k > SA_TOP_MAX_K, flags != 0 (reserved);
 * SA_ERANGE as sa_window_range; SA_ENOMEM when the device scratch (16 bytes a
 * table slot, allocated by the first call) or the result cannot be allocated.
 * The engine stays usable after any error.  Free with sa_top_result_free. */
int sa_window_top(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count,
                  uint32_t flags, sa_top_result **out);
void sa_top_result_free(sa_top_result *r);

/* ---- movers over the window ring ----
 * "Which series fail more now than they did before": the key table is the
 * candidate list, as for sa_window_top, and every candidate is held against
 * the summed cells of two ranges -- a baseline and a current one -- in one
 * pass over the table. */
#define SA_MOVERS_FALL 1u   /* rank by the fall instead of the rise */
typedef struct {
    uint64_t base_first, base_last, cur_first, cur_last;   /* inclusive */
    uint32_t k, n;                  /* asked for; returned (n <= k) */
    uint32_t flags, pad;
    uint64_t n_resident;            /* candidates, as sa_top_result */
    uint64_t n_matched;             /* candidates with score >= max(min_score, 1) */
    uint64_t error_spans_base, error_spans_cur;  /* row 0 of each range's summed cells, exact */
    const uint64_t *key_hash;       /* [n] */
    const int64_t  *score;          /* [n] */
    const uint64_t *baseline;       /* [n] */
    const uint64_t *current;        /* [n] */
} sa_movers_result;

/* Candidates: exactly sa_window_top's -- every non-zero key resident in the
 * key table when the call runs, on every ingest path; on an SA_OPT_DENSE_IDS
 * engine the bound hash, unbound indices not being candidates.  Key 0 and
 * series that got no slot are never candidates.  A reclaim empties the
 * candidates and keeps the cells.
 * Estimates: baseline[i] is bit for bit what sa_window_range(e, base_first,
 * base_last, &key_hash[i], 1, 0, ..) returns in errors[0], current[i] the same
 * for cur_first..cur_last.  Both ranges' windows are folded before any cell is
 * summed.
 * Score: with nb = base_last - base_first + 1 and nc = cur_last - cur_first + 1,
 *   score = current * nb - baseline * nc
 * as a signed 64-bit integer, negated under SA_MOVERS_FALL: the difference of
 * the per-window means, cross-multiplied so that no division or rounding
 * enters (score / (nb * nc) is ERROR spans per window).  Exact while each
 * estimate is below 2^50 -- the largest ring has 4,096 windows, so the
 * products stay below 2^62; beyond that the score is unspecified.
 * Order: the n_matched candidates with score >= max(min_score, 1), sorted by
 * score descending, then key_hash ascending (a total order); the first n =
 * min(k, n_matched) of them are returned, in that order.  min_score >= 2^63
 * matches nothing.
 * Ranges: independent -- each must be resident; they may overlap or be equal.
 * Equal ranges give n_matched == 0 with both counters filled and equal.
 * Ordering and waiting as sa_window_top: joins every launch in flight, runs on
 * the engine stream, waits once, clears nothing (two calls give equal bits).
 * SA_EINVAL for a null `out`, k == 0, k > SA_TOP_MAX_K, flag bits other than
 * SA_MOVERS_FALL; SA_ERANGE for either range as sa_window_range; SA_ENOMEM
 * when the device scratch (sa_window_top's, a second cell array and the rows'
 * estimates, allocated by the first call) or the result cannot be allocated.
 * The engine stays usable after any error.  Free with sa_movers_result_free. */
int sa_window_movers(sa_engine *e, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                     uint64_t cur_last, uint32_t k, uint64_t min_score, uint32_t flags,
                     sa_movers_result **out);
void sa_movers_result_free(sa_movers_result *r);

/* ---- error onset over the window ring ----
 * "Since when has this series been failing": sa_window_movers needs the caller
 * to know where "before" ends and "after" begins; this call tries every split
 * of first..last for every candidate -- one walk over the range's windows with
 * the prefix sums of the key's cells -- and returns the k series whose best
 * split scores highest, each with the window to hold against the deploy log.
 * No state beyond sa_window_top's. */
#define SA_ERROR_ONSET_FALL 1u   /* rank recoveries: the split after which the errors fell most */
typedef struct {
    uint64_t first_window, last_window;   /* the range searched, inclusive */
    uint32_t k, n;                        /* asked for; returned (n <= k) */
    uint32_t flags, pad;
    uint64_t n_resident;            /* candidates, as sa_top_result */
    uint64_t n_eligible;            /* candidates with E >= max(min_count, 1) */
    uint64_t n_matched;             /* eligible candidates whose best D >= max(min_score, 1) */
    uint64_t error_spans;           /* row 0 of the summed cells, as sa_top_result */
    const uint64_t *key_hash;       /* [n] */
    const uint64_t *onset_window;   /* [n] the first window of "after" */
    const int64_t  *score;          /* [n] the best split's D, >= 1 */
    const uint64_t *errors_before;  /* [n] B at the best split */
    const uint64_t *errors_after;   /* [n] A at the best split */
} sa_error_onset_result;

/* Candidates: exactly sa_window_top's -- every non-zero key resident in the
 * key table when the call runs, on every ingest path; on an SA_OPT_DENSE_IDS
 * engine the bound hash, unbound indices not being candidates.  Key 0 and
 * series that got no slot are never candidates.  A reclaim empties the
 * candidates and keeps the cells.
 * Estimates: a key has column c_r = splitmix64(key ^ seed_r) >> shift in row r.
 * With n = last - first + 1 and x_r[j] the cell of window first + j (every
 * window of the range is folded before any cell is read), S_r = the sum of
 * x_r[j] over j and E = min_r S_r: bit for bit what sa_window_range(e, first,
 * last, &key, 1, 0, ..) returns.  A key is eligible when E >= max(min_count, 1).
 * Splits: t in 1 .. n - 1; before is windows first .. first + t - 1, after is
 * first + t .. last.  B(t) = min_r sum_{j<t} x_r[j] and A(t) = min_r (S_r -
 * sum_{j<t} x_r[j]): both are minima of sums, each bit for bit sa_window_range
 * over its side (the two minima may come from different rows).
 * Score: D(t) = A(t) * t - B(t) * (n - t) as a signed 64-bit integer, negated
 * under SA_ERROR_ONSET_FALL: bit for bit the score sa_window_movers gives the
 * key for base = (first, first + t - 1) and cur = (first + t, last), with that
 * call's exactness bound (estimates below 2^50, rings of at most 4,096 windows).
 * Best split: the split with the largest D; among equal D the latest split
 * wins -- deterministic, and it puts the onset on the first failing window
 * after a run of empty ones.  onset_window = first + t.  A range of one window
 * is valid and has no split: n_matched == 0 with the counters filled.
 * Order: a key is matched when it is eligible and its best D >= max(min_score,
 * 1); the matched keys sorted by D descending, then key_hash ascending (the
 * movers' total order); the first n = min(k, n_matched) of them are returned,
 * in that order.  min_score >= 2^63 matches nothing.
 * Ordering and waiting as sa_window_top: joins every launch in flight, folds
 * the range before any cell is read, runs on the engine stream, waits once,
 * clears nothing (two calls give equal bits).
 * SA_EINVAL for a null `out`, k == 0, k > SA_TOP_MAX_K, flag bits other than
 * SA_ERROR_ONSET_FALL; SA_ERANGE as sa_window_range; SA_ENOMEM when the device
 * scratch (sa_window_top's and the rows' splits, allocated by the first call)
 * or the result cannot be allocated.  The engine stays usable after any error.
 * Free with sa_error_onset_result_free. */
int sa_window_error_onset(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count,
                          uint64_t min_score, uint32_t flags, sa_error_onset_result **out);
void sa_error_onset_result_free(sa_error_onset_result *r);

/* ---- service overlap over the window ring ----
 * "How many traces do two services share over these windows": every service's
 * registers are filled from the same hash of the trace id, so the register-wise
 * maximum of two services' arrays is the HLL of the union of their trace sets,
 * and inclusion-exclusion gives the intersection.  The pairwise maxima and
 * their histograms are taken on the device; only the histograms cross the bus. */
#define SA_OVERLAP_MAX_SERVICES 64u
typedef struct {
    uint64_t first_window, last_window;  /* inclusive */
    uint32_t n_sel, n_pairs;             /* n_pairs = n_sel * (n_sel - 1) / 2 */
    uint32_t hll_p, pad;
    const uint32_t *services;   /* [n_sel] service ids, in the caller's order */
    const uint32_t *hll_hist;   /* [n_sel][SA_HLL_HIST_BINS]: as sa_range_result.hll_hist rows */
    const double   *distinct;   /* [n_sel] sa_hll_estimate_hist(hll_hist row, hll_p) */
    const uint32_t *pair_hist;  /* [n_pairs][SA_HLL_HIST_BINS]: value histogram of
                                   max(merged regs of services[i], of services[j]), i < j,
                                   pair index i*n_sel - i*(i+1)/2 + (j-i-1); every row sums to 2^hll_p */
    const double   *union_est;  /* [n_pairs] sa_hll_estimate_hist(pair_hist row, hll_p) */
    const double   *shared;     /* [n_pairs] fmax(0.0, (distinct[i] + distinct[j]) - union_est[pair]) */
} sa_overlap_result;

/* Merge first, then pair: the windows first..last are max-merged per selected
 * service -- exactly the registers sa_window_range returns with
 * SA_RANGE_REGISTERS -- and the pairs are taken on the merged arrays (pairing
 * per window and adding would be wrong: a trace that meets service a in one
 * window and service b in the next is shared).
 * hll_hist / distinct: row i is bit for bit what sa_window_range returns for
 * service services[i].  pair_hist is integer counts; union_est and shared are
 * computed on the host from the histograms in exactly the arithmetic written
 * above, so two calls give equal bits, and an engine and a group give equal
 * bits.
 * Selection: services == NULL with n_sel == 0 selects every service in id
 * order, allowed only when n_services <= SA_OVERLAP_MAX_SERVICES.  n_sel == 1
 * is valid: zero pairs and the one histogram.
 * SA_EINVAL for services == NULL with n_sel == 0 on an engine with more than
 * SA_OVERLAP_MAX_SERVICES services, services == NULL with n_sel != 0, n_sel
 * == 0 with services given, n_sel > SA_OVERLAP_MAX_SERVICES, an id >= n_services, a repeated id, flags != 0
 * (reserved), a null `out`; SA_ERANGE as sa_window_range; SA_ENOMEM when the
 * device scratch (at most n_sel x 2^hll_p bytes plus the histograms, allocated
 * by the first call) or the result cannot be allocated.  The engine stays
 * usable after any error.
 * Ordering and waiting as sa_window_range: joins every launch in flight, runs
 * on the engine stream, waits once, clears nothing.  Works on every ingest
 * path, SA_OPT_DENSE_IDS included: only the registers are read.
 * Accuracy: each of the three estimates (distinct[i], distinct[j], union_est)
 * carries about 1.04 / sqrt(2^hll_p) relative error of its own size, so shared
 * is meaningful only where it is not small against union_est x 1.04 /
 * sqrt(2^hll_p).  The call is exact with respect to the sketches, like
 * sa_window_top.  Free the result with sa_overlap_result_free. */
int sa_window_overlap(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *services,
                      uint32_t n_sel, uint32_t flags, sa_overlap_result **out);
void sa_overlap_result_free(sa_overlap_result *r);

/* ---- duration quantiles over the window ring (SA_OPT_WINDOW_LATENCY) ----
 * "What was checkout's p99 in each of the last 30 windows": per resident
 * window and service the engine keeps a histogram of span durations in
 * SA_LAT_BINS log-linear bins.  Histograms add over windows (and over a
 * group's members), so every output of a sliding series costs one row added
 * and one subtracted, and only counts and quantiles cross the bus.
 *
 * Bin of a duration d = end > start ? end - start : 0 (ns), with q = d >> 7:
 *   q < 16:  bin q                                   (bins 0..15, 128 ns wide)
 *   else:    e = floor(log2 q), bin min(255, ((e - 3) << 3) + (q >> (e - 3)))
 * -- from 2,048 ns up eight bins an octave, each at most 12.5 % wide relative
 * to its lower bound; bin 255 starts at 15 << 37 ns (about 34 min) and has no
 * upper bound (sa_latency_bin_bounds gives UINT64_MAX).
 * Which spans count: exactly those that update their HLL register --
 * service_id < n_services and end_ns / window_ns inside the ring as it stands
 * at the launch.  key_hash is not read: key 0, spans dropped by a full table
 * and unbound dense indices all count. */
#define SA_LAT_BINS  256u
#define SA_LAT_MAX_Q 8u
#define SA_LAT_HIST  1u              /* also return the summed histograms */

typedef struct {
    uint64_t first_window, last_window;  /* outputs t = first..last, inclusive */
    uint32_t width, n_out;               /* output t covers windows t-width+1 .. t; n_out = last-first+1 */
    uint32_t n_sel, n_q;
    const uint32_t *services;   /* [n_sel] service ids, in the caller's order */
    const uint32_t *q_ppm;      /* [n_q] as given */
    const uint64_t *count;      /* [n_out][n_sel] spans of the covered windows */
    const uint8_t  *q_bin;      /* [n_out][n_sel][n_q] the smallest bin whose cumulative count reaches
                                   r = max(1, ceil(count * q_ppm / 10^6)); 0 when count == 0 */
    const uint64_t *q_ns;       /* [n_out][n_sel][n_q] that bin's upper bound (sa_latency_bin_bounds): an
                                   upper bound on the true quantile, within 12.5 % (127 ns in the
                                   linear bins); 0 when count == 0 */
    const uint64_t *hist;       /* [n_out][n_sel][SA_LAT_BINS] the covered windows' bins summed;
                                   NULL without SA_LAT_HIST */
} sa_latency_result;

/* A plain range query is first == last with width = the range's length.
 * services == NULL with n_sel == 0 selects every service in id order.
 * q_ppm[i]: a quantile in parts per million, 1..1000000; 1 <= n_q <=
 * SA_LAT_MAX_Q.  Exact while count < 2^44 (count * q_ppm is taken in u64).
 * Ordering and waiting as sa_window_range: joins every launch in flight, runs
 * on the engine stream, waits once, clears nothing (two calls give equal
 * bits).  Works on every ingest path.
 * SA_ESTATE on an engine without SA_OPT_WINDOW_LATENCY; SA_ERANGE as
 * sa_window_series (first > last, width == 0, width > n_windows, first + 1 <
 * width, or first-width+1 or last not resident); SA_EINVAL for a null `out`,
 * services == NULL with n_sel != 0 or the reverse, an id >= n_services, a
 * repeated id, n_q == 0 or > SA_LAT_MAX_Q, a q_ppm outside 1..10^6, unknown
 * flag bits, n_out * n_sel > 2^20 (> 2^16 with SA_LAT_HIST); SA_ENOMEM when
 * the device scratch or the result cannot be allocated.  While sa_create holds
 * the ring to 2^18 rows, n_out * n_sel cannot pass 2^18, so only the
 * SA_LAT_HIST bound is ever met (128 MiB of histograms a result); the other
 * guards the result's size should the ring's bound move.  The engine stays
 * usable after any error.  Free the result with sa_latency_result_free. */
int sa_window_latency(sa_engine *e, uint64_t first, uint64_t last, uint32_t width, const uint32_t *services,
                      uint32_t n_sel, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                      sa_latency_result **out);
void sa_latency_result_free(sa_latency_result *r);

/* ---- latency movers over the window ring (SA_OPT_WINDOW_LATENCY) ----
 * "Which services got slower": every service is a candidate, and each is held
 * against its own duration histograms summed over two ranges -- a baseline and
 * a current one -- in one pass over the ring; the shift of the ranking
 * quantile's bin is the score.  No state beyond sa_window_latency's. */
#define SA_LATMOV_FALL 1u            /* rank by the fall (speed-ups) instead of the rise */
typedef struct {
    uint64_t base_first, base_last, cur_first, cur_last;  /* inclusive */
    uint32_t k, n;                   /* asked for; returned (n <= k) */
    uint32_t n_q, flags;
    uint64_t n_services;             /* the candidates: every service id 0 .. n_services-1 */
    uint64_t n_eligible;             /* services with count_base >= mc and count_cur >= mc, mc = max(min_count, 1) */
    uint64_t n_matched;              /* eligible services with shift >= max(min_shift, 1) */
    uint64_t spans_base, spans_cur;  /* every service's count summed over each range, exact */
    const uint32_t *q_ppm;           /* [n_q] as given; q_ppm[0] is the ranking quantile */
    const uint32_t *services;        /* [n] */
    const int32_t  *shift;           /* [n] */
    const uint64_t *count_base, *count_cur;   /* [n] */
    const uint8_t  *q_bin_base, *q_bin_cur;   /* [n][n_q] */
    const uint64_t *q_ns_base,  *q_ns_cur;    /* [n][n_q] */
} sa_latency_movers_result;

/* Sums: for every service, Hb is its SA_LAT_BINS-bin rows summed over windows
 * base_first..base_last and Hc the same over cur_first..cur_last -- range
 * sums: the quantile of a sum is not a mean of per-window quantiles --
 * count_base = sum Hb and count_cur = sum Hc.
 * Bins: q_bin_*[i][j] is the smallest bin whose cumulative count reaches
 * max(1, ceil(count * q_ppm[j] / 10^6)) -- exactly sa_window_latency's rule --
 * and q_ns_* that bin's upper bound from sa_latency_bin_bounds.
 * Shift: shift = q_bin_cur[..][0] - q_bin_base[..][0], the sign flipped under
 * SA_LATMOV_FALL, so a returned shift is always >= 1.  From 2,048 ns up 8 bins
 * are a factor of two; below, a bin is 128 ns.  min_shift above 255 matches
 * nothing.
 * Consistency with sa_window_latency: a row's count_base, q_bin_base and
 * q_ns_base are bit for bit what sa_window_latency(e, base_last, base_last,
 * base_last - base_first + 1, &services[i], 1, q_ppm, n_q, 0, ..) returns, and
 * the same holds for cur.
 * Order: the n_matched services -- the eligible ones (count_base >= mc and
 * count_cur >= mc, mc = max(min_count, 1)) with shift >= max(min_shift, 1) --
 * sorted by shift descending, then count_cur descending (among equally shifted
 * services the busiest first; for ordering count_cur is clamped at 2^48 - 1),
 * then service id ascending: a total order.  The first n = min(k, n_matched)
 * are returned, in that order.  Exact while counts stay below 2^44, as
 * sa_window_latency.  Service id 0 is an ordinary candidate.
 * Ranges: independent -- each must be resident; they may overlap, be equal, or
 * have base after cur.  Equal ranges give n_matched == 0 with n_eligible and
 * both spans_* filled and equal.
 * Ordering and waiting as sa_window_movers: joins every launch in flight, runs
 * on the engine stream, waits once, clears nothing (two calls give equal
 * bits).  Works on every ingest path: only the latency ring is read.
 * SA_ESTATE on an engine without SA_OPT_WINDOW_LATENCY; SA_ERANGE for either
 * range as sa_window_range; SA_EINVAL for a null `out`, k == 0, k >
 * SA_TOP_MAX_K, n_q == 0 or > SA_LAT_MAX_Q, a null q_ppm, a q_ppm outside
 * 1..10^6, flag bits other than SA_LATMOV_FALL; SA_ENOMEM when the device
 * scratch (both ranges' sums, 2 x n_services x 2 KiB, the candidates, 16 B a
 * service, and the select's state, allocated by the first call) or the result
 * cannot be allocated.  The engine stays usable after any error.  Free with
 * sa_latency_movers_result_free. */
int sa_window_latency_movers(sa_engine *e, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                             uint64_t cur_last, uint32_t k, uint64_t min_count, uint32_t min_shift,
                             const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                             sa_latency_movers_result **out);
void sa_latency_movers_result_free(sa_latency_movers_result *r);

/* ---- latency SLO burn over sliding widths (SA_OPT_WINDOW_LATENCY) ----
 * "What share of checkout's requests were slower than its target over the last
 * 5 minutes and over the last hour, at every window, and is the error budget
 * burning": the multi-window, multi-burn-rate alert.  A threshold turns a
 * service's SA_LAT_BINS-bin row into a (total, slow) pair, so every width
 * slides over 16 bytes a window, the ring is read once whatever the widths,
 * and only the pairs' sums and the verdicts cross the bus.  No state beyond
 * sa_window_latency's. */
#define SA_SLO_MAX_WIDTHS 4u
typedef struct {
    uint64_t first_window, last_window;   /* outputs t = first..last, inclusive */
    uint32_t n_out, n_sel, n_widths, pad;
    uint64_t min_count;                   /* as applied: max(min_count, 1) */
    const uint32_t *services;      /* [n_sel] ids, in the caller's order */
    const uint32_t *widths;        /* [n_widths] as given */
    const uint32_t *limit_ppm;     /* [n_widths] as given */
    const uint64_t *threshold_ns;  /* [n_sel] as given */
    const uint8_t  *threshold_bin; /* [n_sel] sa_latency_bin(threshold_ns[i]) */
    const uint64_t *effective_ns;  /* [n_sel] that bin's upper bound: "slow" means d > effective_ns */
    const uint64_t *total;         /* [n_out][n_widths][n_sel] spans of windows t-widths[w]+1 .. t */
    const uint64_t *slow;          /* [n_out][n_widths][n_sel] of those, spans in bins > threshold_bin */
    const uint8_t  *burning;       /* [n_out][n_sel] bit w set when width w burns (below) */
    const uint32_t *alert_outputs; /* [n_sel] outputs whose n_widths low bits are all set */
} sa_slo_result;

/* Slow: with b = sa_latency_bin(threshold_ns[i]), a span of service
 * services[i] is slow when its bin is greater than b; spans in bin b itself
 * count as fast.  So `slow` counts exactly the spans with d > effective_ns,
 * the upper bound of bin b: exact with respect to the caller's threshold when
 * that is a bin's upper bound from sa_latency_bin_bounds, else a lower bound
 * within one bin (12.5 %).  A threshold in bin 255 makes `slow` 0 everywhere.
 * Counts: total[t][w][i] is bit for bit the count of sa_window_latency(e, t,
 * t, widths[w], &services[i], 1, ..), and slow[t][w][i] the sum of that call's
 * SA_LAT_HIST row over the bins above threshold_bin[i].  Which spans count is
 * sa_window_latency's rule.
 * Burn: width w burns at (t, i) when total >= max(min_count, 1) and slow *
 * 10^6 > limit_ppm[w] * total -- strictly; both products are taken in u64 and
 * are exact while counts stay below 2^44, sa_window_latency's bound.  The
 * caller folds objective and burn factor into limit_ppm: a 99.9 % objective
 * at burn 14.4 is 14,400.  alert_outputs[i] counts the outputs at which every
 * asked width burns: the long-and-short-window rule.
 * Arguments: 1 <= n_widths <= SA_SLO_MAX_WIDTHS; widths and limit_ppm
 * non-null, every limit_ppm in 0..10^6; widths in any order, repeats allowed.
 * The selection as sa_window_latency's: services == NULL with n_sel == 0
 * selects every service in id order.  threshold_ns is non-null and parallel
 * to the selection (n_services entries when every service is selected); any
 * u64 passes.  flags are reserved (0).  n_out * n_sel <= 2^20.
 * Ordering and waiting as sa_window_latency: joins every launch in flight,
 * runs on the engine stream, waits once, clears nothing (two calls give equal
 * bits).  Works on every ingest path: only the latency ring is read.
 * SA_ESTATE on an engine without SA_OPT_WINDOW_LATENCY; SA_ERANGE when any
 * width fails sa_window_series' span rule against first..last (every window
 * first - max(widths) + 1 .. last resident, each width in 1..n_windows);
 * SA_EINVAL for the argument rules above and a null `out`; SA_ENOMEM when the
 * device scratch (16 B a covered window and service, twice, and the answers)
 * or the result cannot be allocated.  The engine stays usable after any
 * error.  Free the result with sa_slo_result_free. */
int sa_window_slo(sa_engine *e, uint64_t first, uint64_t last, const uint32_t *widths,
                  const uint32_t *limit_ppm, uint32_t n_widths, const uint32_t *services, uint32_t n_sel,
                  const uint64_t *threshold_ns, uint64_t min_count, uint32_t flags, sa_slo_result **out);
void sa_slo_result_free(sa_slo_result *r);

/* ---- latency onset over the window ring (SA_OPT_WINDOW_LATENCY) ----
 * "Since when": sa_window_latency_movers and sa_window_slo need the caller to
 * know where "before" ends and "after" begins; this call finds that window for
 * every service -- the change point of its slow share over first..last, the
 * maximum of a CUSUM over the prefix sums of its (total, slow) pairs -- and
 * returns the k services whose slow share changed most, each with the window
 * to hold against the deploy log.  One call, the ring read at most twice.  No
 * state beyond sa_window_latency's. */
#define SA_ONSET_FALL 1u   /* rank speed-ups: the slow share fell */
typedef struct {
    uint64_t first_window, last_window;   /* the range searched, inclusive */
    uint32_t k, n;                        /* asked for; returned (n <= k) */
    uint32_t flags, q_ppm;                /* q_ppm as given (0 when threshold_ns was given) */
    uint64_t min_count;                   /* as applied: max(min_count, 1) */
    uint64_t n_services, n_eligible, n_matched;
    uint64_t spans;                       /* every service's count over the range, exact */
    const uint32_t *services;       /* [n] */
    const uint64_t *onset_window;   /* [n] the first window of "after" */
    const int32_t  *delta_ppm;      /* [n] >= 1 */
    const uint8_t  *threshold_bin;  /* [n] */
    const uint64_t *effective_ns;   /* [n] that bin's upper bound */
    const uint64_t *total_before, *slow_before, *total_after, *slow_after;  /* [n] */
} sa_onset_result;

/* Threshold: every service s is cut at a bin b_s.  With threshold_ns != NULL
 * the array has n_services entries, any u64 passes, and b_s =
 * sa_latency_bin(threshold_ns[s]) -- sa_window_slo's rule; q_ppm must then be
 * 0.  With threshold_ns == NULL, q_ppm must be in 1..10^6 and b_s is the
 * quantile bin of the service's rows summed over first..last by
 * sa_window_latency's rule: the smallest bin whose cumulative count reaches
 * max(1, ceil(count * q_ppm / 10^6)) (0 for a service without spans) -- the
 * pooled quantile: no prior is needed.  A span is slow when its bin is > b_s;
 * effective_ns is the upper bound of bin b_s.
 * Pairs and splits: n_cov = last - first + 1, and window first + j gives
 * (tot_j, slow_j).  A split is t in 1 .. n_cov - 1: before is windows first ..
 * first + t - 1, after is first + t .. last.  N_b, S_b, N_a, S_a are the sums
 * of the two sides, N and S those of the whole range.  A split is eligible when
 * N_b >= mc and N_a >= mc, mc = max(min_count, 1).  A range of one window is
 * valid and has no split: n_eligible == 0.
 * Statistic: D(t) = S_a * N_b - S_b * N_a (= S * N_b - N * S_b), negated under
 * SA_ONSET_FALL, taken as a signed 128-bit integer: exact while a service's
 * count over the range stays below 2^44, sa_window_latency's bound (the
 * products reach 2^88).
 * Best split: the eligible split with the largest D; among equal D the latest
 * split wins -- deterministic, and it puts the onset on the first non-empty
 * window after a run of empty ones.  onset_window = first + t.
 * Delta: delta_ppm = floor(S_a * 10^6 / N_a) - floor(S_b * 10^6 / N_b) at the
 * best split, negated under SA_ONSET_FALL; both quotients are taken in u64.
 * Counters: a service is eligible when it has at least one eligible split
 * (n_eligible), and matched when it is eligible, its best D > 0 and delta_ppm
 * >= max(min_delta_ppm, 1) (n_matched).  A min_delta_ppm above 10^6 matches
 * nothing.  spans sums N over every service.
 * Order: the matched services sorted by delta_ppm descending, then N
 * descending (clamped at 2^44 - 1 for ordering), then service id ascending: a
 * total order.  The first n = min(k, n_matched) are returned, in that order.
 * Consistency with sa_window_slo: a row's total_before and slow_before are bit
 * for bit the total and slow of sa_window_slo(e, onset - 1, onset - 1, {onset -
 * first}, .., &service, 1, &effective_ns, ..), and total_after and slow_after
 * those of the call at (last, last, {last - onset + 1}).
 * Ordering and waiting as sa_window_latency_movers: joins every launch in
 * flight, runs on the engine stream, waits once, clears nothing (two calls
 * give equal bits).  Works on every ingest path: only the latency ring is read.
 * SA_ESTATE on an engine without SA_OPT_WINDOW_LATENCY; SA_ERANGE as
 * sa_window_range; SA_EINVAL for a null `out`, k == 0, k > SA_TOP_MAX_K, flag
 * bits other than SA_ONSET_FALL, threshold_ns == NULL with q_ppm outside
 * 1..10^6, threshold_ns != NULL with q_ppm != 0; SA_ENOMEM when the device
 * scratch (the pooled sums, n_services x 2 KiB, the pairs, 16 B a window and
 * service, 40 B and a candidate a service, and the select's state, allocated by
 * the first call) or the result cannot be allocated.  The engine stays usable
 * after any error.  Free with sa_onset_result_free. */
int sa_window_latency_onset(sa_engine *e, uint64_t first, uint64_t last, uint32_t k, uint32_t q_ppm,
                            const uint64_t *threshold_ns, uint64_t min_count, uint32_t min_delta_ppm,
                            uint32_t flags, sa_onset_result **out);
void sa_onset_result_free(sa_onset_result *r);

int sa_get_stats(sa_engine *e, sa_stats *out);

/* ---- multi-GPU merge hooks (device pointers on this engine's device) ----
 * Used by the host's RCCL merge: gather the local key list, build the sorted
 * union across ranks, densify local counters against it, all-reduce. */
/* Folds pending partials into the HBM table and writes the resident keys that
 * have a non-zero delta into d_keys (capacity `cap`); *n_out = count (may exceed
 * cap, in which case nothing beyond cap is written). */
/* SA_OPT_DENSE_IDS engines: declares that index[j] is series key_hash[j]
 * (host arrays, borrowed for the call).  Ordered on the engine stream before
 * every later ingest on any stream.  SA_EINVAL for an index of 0 or >=
 * table_capacity and for a key_hash of 0; SA_ESTATE on an engine without the
 * option.  Binding an index that is already bound recycles it: allowed only
 * with no spans ingested since the last flush (SA_ESTATE otherwise); every
 * resident window's ERROR counts of the old series go to its count-min cells
 * first, so the old series keeps its errors. */
int sa_bind_ids(sa_engine *e, const uint64_t *index, const uint64_t *key_hash, uint64_t n);
int sa_export_keys(sa_engine *e, uint64_t *d_keys, uint64_t cap, uint64_t *n_out, void *stream);
/* d_rows[i] = [bucket counts..., sum_ns] (n_buckets+1 u64) for d_keys[i]
 * (zeros if absent). reset != 0 clears the engine's delta counters afterwards. */
int sa_gather_dense(sa_engine *e, const uint64_t *d_keys, uint64_t n, uint64_t *d_rows,
                    int reset, void *stream);
/* Window sketches into device buffers: d_hll [n_services][2^p] u8 and
 * d_cms [d][w] u64 (unsaturated, for sum all-reduce). */
int sa_window_export(sa_engine *e, uint64_t window_id, uint8_t *d_hll, uint64_t *d_cms,
                     void *stream);

/* ---- engine groups: one engine per GPU behind one handle ----
 * The connector's single ConsumeTraces/exportMetrics pair over several GPUs.
 * Spans shard by trace id (engine = trace_w1 % n), so every trace's spans land
 * on one engine and the per-engine sketches stay exact partials; the group's
 * flush / window read return the merge:
 *   RED: key union across engines (a series seen on several engines is one
 *        row), bucket counts and ns sums added;
 *   HLL: registers max-merged (exact and idempotent);
 *   count-min: cells added, then saturated to u32.
 * Merge transport: when every member has its own device the group owns an
 * RCCL communicator over them (ncclAllGather of the key lists, ncclAllReduce
 * sum u64 of the dense rows and count-min cells, max u8 of the HLL
 * registers, over xGMI); members that share a device (or SA_OPT_GROUP_COPY)
 * merge through device-to-device copies onto member 0's device and a reduce
 * kernel there.  Results are identical either way (integer sums and maxima).
 * Threading: as an engine (single producer); sa_group_ingest fans the shards
 * out to one host thread per member. */
typedef struct sa_group sa_group;
/* devices[i] = HIP ordinal of member i (repeats allowed); cfg->device is ignored. */
int sa_group_create(const sa_config *cfg, const int32_t *devices, uint32_t n, sa_group **out);
void sa_group_destroy(sa_group *g);
const char *sa_group_last_error(const sa_group *g);
uint32_t sa_group_size(const sa_group *g);
/* 1 when the group merges over RCCL, 0 when through device copies */
int sa_group_uses_rccl(const sa_group *g);
/* Member engine i (for device-resident ingest of a shard the caller made). */
sa_engine *sa_group_member(sa_group *g, uint32_t i);
/* Host batch: split by trace_w1 % n, each shard ingested by its member.  The
 * split is one pass over trace_w1 (shard sizes) and one gather of each span
 * into its member's packed shard, both on worker threads; the call returns
 * once every member has copied its shard out of the caller's buffers. */
int sa_group_ingest(sa_group *g, const sa_span_batch *batch);
/* Device-resident batch in HBM of member `src`'s device (`stream`: a
 * hipStream_t of that device, NULL = the group's stream there).  A partition
 * kernel on that device counts the shards (trace_w1 % n; the call waits for
 * these counts, a few microseconds) and scatters every span into its member's
 * packed shard; shards of members on other devices are copied there
 * peer-to-peer (xGMI DMA), and every member ingests its shard on its own
 * stream.  Asynchronous otherwise: the batch must stay valid until `stream`
 * reaches this point (the partition has read it); sa_group_sync waits for the
 * members.  Same results as sa_group_ingest of the same spans. */
int sa_group_ingest_device(sa_group *g, const sa_span_batch *batch, uint32_t src, void *stream);
int sa_group_sync(sa_group *g);
/* Merged delta since the previous group flush (members reset); SA_EFULL as
 * sa_flush when any member dropped spans. Free with sa_red_result_free. */
int sa_group_flush(sa_group *g, sa_red_result **out);
/* exportMetrics of a group built with exp_max_size != 0: the members' delta
 * exponential histograms folded per series (the histogram one engine fed
 * every member's spans would hold). Free with sa_exp_result_free. */
int sa_group_flush_exp(sa_group *g, sa_exp_result **out);
/* Merged sketches of one resident window. Free with sa_sketch_result_free. */
int sa_group_window_read(sa_group *g, uint64_t window_id, sa_sketch_result **out);
int sa_group_window_advance(sa_group *g, uint64_t new_base);
/* sa_window_range of a group: every member merges its own windows on its
 * device, the group's transport merges the members' registers (max) and
 * cells (sum), and member 0's device takes the histogram and the point
 * queries.  Results equal those of one engine fed every span. */
int sa_group_window_range(sa_group *g, uint64_t first, uint64_t last, const uint64_t *keys,
                          uint64_t n_keys, uint32_t flags, sa_range_result **out);
/* sa_window_top of a group: the members merge their cells as for
 * sa_group_window_range, every member scans its own key table against the
 * merged cells (an estimate depends on the key and the merged cells only, so
 * the group's first k are among the members' first k), and the host drops the
 * repeats and cuts to k in the same order.  key_hash / errors equal those of
 * one engine fed every span; n_resident and n_matched are summed over members
 * (a series on several members counts once per member, as n_keys of
 * sa_group_get_stats does). */
int sa_group_window_top(sa_group *g, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count,
                        uint32_t flags, sa_top_result **out);
/* sa_window_movers of a group: every member sums both ranges on its device,
 * the transport sums both cell arrays across members and leaves the sums on
 * every member, every member scans its own key table against the merged
 * arrays (a score depends on the key and the merged cells only, so the
 * group's first k are among the members' first k), and the host drops the
 * repeats and cuts to k in the same order.  The rows and both error_spans_*
 * equal those of one engine fed every span; n_resident and n_matched are
 * summed over members, as in sa_group_window_top. */
int sa_group_window_movers(sa_group *g, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                           uint64_t cur_last, uint32_t k, uint64_t min_score, uint32_t flags,
                           sa_movers_result **out);
/* sa_window_error_onset of a group: every member exports the cells of every
 * window of the range -- not their sum: n x d x w x 8 bytes a member, SA_ENOMEM
 * when that does not fit -- the transport sums the arrays across members and
 * leaves the sums on every member, every member scans its own key table
 * against the merged windows (a row depends on the key and the merged cells
 * only), and the host drops the repeats and cuts to k in the same order.  The
 * rows and error_spans equal those of one engine fed every span; n_resident,
 * n_eligible and n_matched are summed over members, as in sa_group_window_top. */
int sa_group_window_error_onset(sa_group *g, uint64_t first, uint64_t last, uint32_t k, uint64_t min_count,
                                uint64_t min_score, uint32_t flags, sa_error_onset_result **out);
/* sa_window_overlap of a group: every member max-merges its own windows on
 * its device, the group's transport merges the members' registers (max, every
 * service's rows as for sa_group_window_range), and member 0's device gathers
 * the selected rows and takes the pairwise maxima.  Results equal those of one
 * engine fed every span, bit for bit. */
int sa_group_window_overlap(sa_group *g, uint64_t first, uint64_t last, const uint32_t *services,
                            uint32_t n_sel, uint32_t flags, sa_overlap_result **out);
/* sa_window_latency of a group: every member takes the sliding sums of its
 * own ring on its device, the group's transport adds the members' sums
 * (histograms are additive over members), and member 0's device takes the
 * counts and the quantile bins.  Results equal those of one engine fed every
 * span, bit for bit.  Every member's sums of a call take n_out * n_sel * 2 KiB
 * on its device: at most the ring's own size, 512 MiB. */
int sa_group_window_latency(sa_group *g, uint64_t first, uint64_t last, uint32_t width, const uint32_t *services,
                            uint32_t n_sel, const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                            sa_latency_result **out);
/* sa_window_latency_movers of a group: every member sums both ranges of its
 * own ring on its device, the group's transport adds the members' sums
 * (histograms are additive over members), and member 0's device scores,
 * selects and reads the rows.  Results equal those of one engine fed every
 * span, bit for bit.  Every member's sums of a call take 2 x n_services x 2 KiB
 * on its device. */
int sa_group_window_latency_movers(sa_group *g, uint64_t base_first, uint64_t base_last, uint64_t cur_first,
                                   uint64_t cur_last, uint32_t k, uint64_t min_count, uint32_t min_shift,
                                   const uint32_t *q_ppm, uint32_t n_q, uint32_t flags,
                                   sa_latency_movers_result **out);
/* sa_window_slo of a group: every member reduces its own ring's covered rows
 * to (total, slow) pairs on its device, the group's transport adds the
 * members' pairs (16 B a covered window and service), and member 0's device
 * slides every width over the sums and judges.  Results equal those of one
 * engine fed every span, bit for bit. */
int sa_group_window_slo(sa_group *g, uint64_t first, uint64_t last, const uint32_t *widths,
                        const uint32_t *limit_ppm, uint32_t n_widths, const uint32_t *services, uint32_t n_sel,
                        const uint64_t *threshold_ns, uint64_t min_count, uint32_t flags, sa_slo_result **out);
/* sa_window_latency_onset of a group, in two rounds of the transport.  With a
 * pooled threshold every member first sums the range of its own ring per
 * service, the transport adds the members' sums and leaves them on every
 * member, and each member takes the same threshold bins from them (with
 * threshold_ns given this round is skipped).  Then every member cuts its rows
 * to (total, slow) pairs, the transport adds the pairs, and member 0's device
 * scans, selects and reads the rows.  Results equal those of one engine fed
 * every span, bit for bit. */
int sa_group_window_latency_onset(sa_group *g, uint64_t first, uint64_t last, uint32_t k, uint32_t q_ppm,
                                  const uint64_t *threshold_ns, uint64_t min_count, uint32_t min_delta_ppm,
                                  uint32_t flags, sa_onset_result **out);
/* Counters summed over members (n_keys and table_capacity too; window_base and
 * small_table from member 0). */
int sa_group_get_stats(sa_group *g, sa_stats *out);

/* ---- pure host helpers (no device needed) ---- */
/* Integer bucket thresholds: bucket(d_ns) = n_neg + #{i : d_ns > thr[i]} equals
 * sort.SearchFloat64s(bounds, float64(d_ns)/div) for every u64 d_ns. Returns
 * n_neg via *n_neg and fills thr[0 .. n_bounds-n_neg). */
int sa_bucket_thresholds(const double *bounds, uint32_t n_bounds, uint32_t unit,
                         uint64_t *thr, uint32_t *n_neg);
/* HLL estimate of one register array (standard estimator + linear counting). */
double sa_hll_estimate(const uint8_t *regs, uint32_t p);
/* The same estimate from a register array's value histogram (hist[v] =
 * registers holding v, SA_HLL_HIST_BINS words summing to 2^p): sum hist[v] *
 * 2^-v is taken exactly, as sum hist[v] << (63 - v) in a 128-bit integer
 * converted to double once, so the result does not depend on any summation
 * order; then sa_hll_estimate's alpha and linear-counting branch (zeros =
 * hist[0]).  -1.0 for p outside 4..18.  Defines sa_range_result.distinct. */
double sa_hll_estimate_hist(const uint32_t *hist, uint32_t p);
/* The latency bin of a duration in ns (the rule above sa_latency_result). */
uint32_t sa_latency_bin(uint64_t d_ns);
/* The durations of one bin, inclusive: for bin < 16 [bin << 7, (bin << 7) +
 * 127]; else with e = (bin >> 3) + 2 and m = bin & 7, lo = ((8 + m) << (e -
 * 3)) << 7 and hi = (((9 + m) << (e - 3)) << 7) - 1; hi of bin 255 is
 * UINT64_MAX.  The bins tile [0, 2^64).  SA_EINVAL for bin >= SA_LAT_BINS or a
 * null pointer. */
int sa_latency_bin_bounds(uint32_t bin, uint64_t *lo, uint64_t *hi);

#ifdef __cplusplus
}
#endif
#endif
