/*
 * spanagg_diag.h -- test and profiling entry points of libspanagg.
 *
 * These are not connector operations and replace nothing in the reference:
 * the parity tests use them to check single kernel stages (the exponential
 * bucket index, the group's device key union) against numpy / the oracle, and
 * the profiling tools read per-workgroup timestamps.  The drop-in boundary is
 * include/spanagg.h, which does not include this header; a collector binding
 *  never needs it.
 */
#ifndef SPANAGG_DIAG_H
#define SPANAGG_DIAG_H
#include "spanagg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic: out[i] = the exponential bucket index of v[i] at scale[i] and
 * logs[i] = Go's math.Log(v[i]), both computed on the engine's GPU
 * (host arrays; n <= 2^20). */
int sa_expo_probe(sa_engine *e, const double *v, const int32_t *scale, uint64_t n, int32_t *out, double *logs);
/* Diagnostic: the bucket-index fast path the counting kernel uses.  For each
 * duration d_ns[i] > 0 at scale[i]: exact[i] = the Go-exact index of
 * d_ns / (1e6 or 1e9 by the engine's unit), fast[i] = the fast path's index
 * or INT32_MIN when it defers to the exact path (host arrays; n <= 2^20).
 * *log2_err (may be null) = max |v_log_f32(m) - log2(m)| over every float m
 * in [1, 2), the bound the fast path's margins assume. */
int sa_expo_fast_probe(sa_engine *e, const uint64_t *d_ns, const int32_t *scale, uint64_t n, int32_t *fast,
                       int32_t *exact, double *log2_err);

/* Diagnostic: the device key union the group flush builds (sa::key_union:
 * bucket sort by the top bits, bitonic per bucket, repeats and 0 dropped) on
 * the engine's GPU.  out[0 .. *n_out) = the distinct non-zero ids of
 * in[0 .. n) ascending (host arrays; out holds n; n <= 2^28). */
int sa_key_union_probe(sa_engine *e, const uint64_t *in, uint64_t n, uint64_t *out, uint64_t *n_out);

/* Diagnostic: sa_window_latency_onset's scan, select and rows on the caller's
 * own pairs (host, [n_sel][n_cov][2] u64: service i's window j as {total,
 * slow}) instead of a ring's: the only way to reach the 128-bit arithmetic --
 * counts near 2^43 -- in a test that takes seconds.  The result reads as
 * sa_window_latency_onset's with first_window 0, last_window n_cov - 1,
 * n_services n_sel and q_ppm 0; threshold_bin and effective_ns come back 0.
 * Any engine serves (the ring is not read).  SA_EINVAL for a null pointer,
 * n_sel or n_cov of 0, n_sel * n_cov > 2^18, and k and flags as
 * sa_window_latency_onset.  Free with sa_onset_result_free. */
int sa_onset_probe(sa_engine *e, const uint64_t *pairs, uint32_t n_sel, uint32_t n_cov, uint32_t k,
                   uint64_t min_count, uint32_t min_delta_ppm, uint32_t flags, sa_onset_result **out);

/* Diagnostic only: per-workgroup s_memrealtime stamps (100 MHz) of the last
 * small-table ingest launch, [G][136] = {start, after LDS setup, after the span
 * loop, after the slab flush, 0 x 4, then per wave 8 segment cycle sums};
 * filled only when the engine was created with SA_OPT_STAMPS (*n_out = 0
 * otherwise). */
int sa_debug_stamps(sa_engine *e, uint64_t *out, uint64_t cap, uint64_t *n_out);

/* Which ingest kernel an engine runs (sa_debug_geometry_info.kernel).  Small
 * tables: the kernel specialised for the default geometry (2,048 slots, 17
 * buckets, HLL p = 14), the generic kernel with 512- or 1,024-thread
 * workgroups, or the linear-threshold kernel for bounds no bin table holds.
 * Small exponential tables: the kernel specialised for 2,048 slots and p = 14,
 * or the generic one.  HBM tables (exponential, binned, dense, partitioned,
 * atomic): the instance for 16 non-negative bounds or the generic one (the
 * binned and dense scatters have a single instance; the value then only names
 * the bounds).  SA_KERNEL_LAB: a laboratory variant (libspanagg_ab.so). */
enum {
  SA_KERNEL_SMALL_DEFAULT = 0,
  SA_KERNEL_SMALL_512 = 1,
  SA_KERNEL_SMALL_1024 = 2,
  SA_KERNEL_SMALL_LINEAR = 3,
  SA_KERNEL_EXPO_SPECIALISED = 4,
  SA_KERNEL_EXPO_GENERIC = 5,
  SA_KERNEL_BOUNDS16 = 6,
  SA_KERNEL_BOUNDS_GENERIC = 7,
  SA_KERNEL_LAB = 8
};

typedef struct sa_debug_geometry_info {
  uint32_t path;        /* 0 Small, 1 ExpoSmall, 2 ExpoHbm, 3 Binned, 4 Dense, 5 Partitioned, 6 Atomic */
  uint32_t kernel;      /* SA_KERNEL_* */
  uint32_t block;       /* threads per ingest workgroup */
  uint32_t grid_max;    /* G: the most workgroups one ingest launch uses */
  uint32_t log2cap;     /* log2 of the key table's slots */
  uint32_t lb_shift;    /* HLL lower-bound filter: sub-blocks of 2^lb_shift registers ... */
  uint32_t lb_n;        /* ... lb_n of them; 0: the filter is off */
  uint32_t error_table; /* 1: per-workgroup (window, slot) ERROR tables (small tables) */
  uint64_t lds_bytes;   /* the ingest kernel's dynamic LDS (small tables) */
  /* the exponential histograms' counting pass (all 0 without exp_max_size) */
  uint32_t expo_count;     /* SA_EXPO_COUNT_*: which kernels count the buckets */
  uint32_t expo_entries;   /* slab counting: a counting workgroup's LDS entries; cached-probe: its cache's; else 0 */
  uint32_t expo_bin_slots; /* slab counting: key slots per fold bin of the tail records (16, 8 past max_size 2,048) */
  uint32_t expo_bins;      /* slab counting: fold bins (slots / expo_bin_slots, rounded up) */
} sa_debug_geometry_info;

/* How an exponential engine counts buckets (sa_debug_geometry_info.expo_count).
 * Small tables: slab counting (a series among the expo_entries most frequent
 * of the last launch counts in LDS, the others leave as tail records that one
 * workgroup per fold bin adds up), or with SA_OPT_EXPO_CACHED -- and when the
 * LDS has no room for one entry -- the cached-probe kernel.  HBM tables
 * (SA_OPT_EXPO_HBM, or more slots than LDS holds): the three HBM passes. */
enum { SA_EXPO_COUNT_NONE = 0, SA_EXPO_COUNT_SLAB = 1, SA_EXPO_COUNT_CACHED = 2, SA_EXPO_COUNT_HBM = 3 };

/* Diagnostic: the geometry decisions sa_create took for this engine, so a
 * test can assert which device code it is about to run: the ingest kernel and
 * its launch geometry, the HLL filter, the ERROR table, and for exponential
 * histograms the counting kernel (expo_count), its LDS entries (expo_entries)
 * and the tail fold's layout (expo_bin_slots, expo_bins).  Host state only. */
int sa_debug_geometry(sa_engine *e,sa_debug_geometry_info *out);

#ifdef __cplusplus
}
#endif
#endif
