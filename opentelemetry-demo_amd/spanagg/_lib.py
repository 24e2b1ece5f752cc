"""ctypes binding of libspanagg's C-ABI (include/spanagg.h).

The shared library is built in-tree (``make -C opentelemetry-demo_amd``) next to
this file.  There is no fallback: if the library is missing, ``load()`` raises,
and if no gfx950 device is present ``sa_create`` fails with SA_EDEVICE.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SPANAGG_LIB: another build of the same ABI -- libspanagg_ab.so, the laboratory
# build tools/ use for A/B variants and ablations (`make -C opentelemetry-demo_amd ab`)
LIB_PATH = os.environ.get("SPANAGG_LIB") or os.path.join(_HERE, "libspanagg.so")

SA_OK, SA_EINVAL, SA_ENOMEM, SA_EDEVICE, SA_EFULL, SA_ERANGE, SA_ESTATE = 0, -1, -2, -3, -4, -5, -6
SA_UNIT_MS, SA_UNIT_S = 0, 1
SA_MAX_BOUNDS = 62
# sa_config.options (include/spanagg.h SA_OPT_*): alternative kernel paths with
# the same results, for parity tests and A/B runs
OPT_NO_HLL_FILTER, OPT_PARTITIONED, OPT_ATOMIC_TABLE, OPT_EXPO_HBM, OPT_EXPO_CACHED = 1, 2, 4, 8, 16
OPT_IDENTITY_IDS, OPT_STAMPS, OPT_GROUP_COPY, OPT_GROUP_RCCL = 32, 64, 128, 256
# the key_hash column carries dense series indices (spanagg.dense.DenseIds, Engine.bind_ids)
OPT_DENSE_IDS = 512
# per window and service a 256-bin histogram of durations beside every ingest path (Engine.window_latency)
OPT_WINDOW_LATENCY = 1024
STATUS_NAMES = {
    SA_OK: "SA_OK", SA_EINVAL: "SA_EINVAL", SA_ENOMEM: "SA_ENOMEM", SA_EDEVICE: "SA_EDEVICE",
    SA_EFULL: "SA_EFULL", SA_ERANGE: "SA_ERANGE", SA_ESTATE: "SA_ESTATE",
}

u64p = C.POINTER(C.c_uint64)
u32p = C.POINTER(C.c_uint32)
u8p = C.POINTER(C.c_uint8)
f64p = C.POINTER(C.c_double)


class sa_config(C.Structure):
    _fields_ = [
        ("bounds", f64p), ("n_bounds", C.c_uint32), ("unit", C.c_uint32),
        ("hll_p", C.c_uint32), ("cms_d", C.c_uint32), ("cms_w", C.c_uint32),
        ("window_ns", C.c_uint64), ("n_windows", C.c_uint32), ("n_services", C.c_uint32),
        ("key_capacity", C.c_uint64), ("device", C.c_int32), ("flags", C.c_uint32),
        ("exp_max_size", C.c_uint32), ("options", C.c_uint32),
    ]


class sa_span_batch(C.Structure):
    _fields_ = [
        ("key_hash", C.c_void_p), ("start_ns", C.c_void_p), ("end_ns", C.c_void_p),
        ("trace_w0", C.c_void_p), ("trace_w1", C.c_void_p), ("meta", C.c_void_p),
        ("n", C.c_uint64),
    ]


class sa_red_result(C.Structure):
    _fields_ = [
        ("n_series", C.c_uint64), ("n_buckets", C.c_uint32),
        ("key_hash", u64p), ("bucket_counts", u64p), ("calls", u64p),
        ("sum_ns", u64p), ("sum", f64p),
    ]


class sa_exp_result(C.Structure):
    _fields_ = [
        ("n_series", C.c_uint64), ("max_size", C.c_uint32), ("unit", C.c_uint32),
        ("key_hash", u64p), ("count", u64p), ("zero_count", u64p), ("sum_ns", u64p),
        ("sum", f64p), ("min", f64p), ("max", f64p),
        ("scale", C.POINTER(C.c_int32)), ("offset", C.POINTER(C.c_int32)), ("n_buckets", u32p),
        ("bucket_counts", u64p),
    ]


class sa_sketch_result(C.Structure):
    _fields_ = [
        ("window_id", C.c_uint64), ("n_services", C.c_uint32), ("hll_p", C.c_uint32),
        ("hll", u8p), ("cms_d", C.c_uint32), ("cms_w", C.c_uint32), ("cms", u32p),
    ]


SA_HLL_HIST_BINS = 64
SA_RANGE_REGISTERS, SA_RANGE_CELLS = 1, 2


class sa_range_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("n_services", C.c_uint32), ("hll_p", C.c_uint32),
        ("hll_hist", u32p), ("distinct", f64p), ("hll", u8p), ("cms_d", C.c_uint32), ("cms_w", C.c_uint32),
        ("cms", u64p), ("n_keys", C.c_uint64), ("errors", u64p),
    ]


class sa_series_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("width", C.c_uint32), ("n_out", C.c_uint32),
        ("n_services", C.c_uint32), ("hll_p", C.c_uint32), ("hll_hist", u32p), ("distinct", f64p),
        ("error_spans", u64p), ("n_keys", C.c_uint64), ("errors", u64p),
    ]


SA_TOP_MAX_K = TOP_MAX_K = 4096


class sa_top_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("k", C.c_uint32), ("n", C.c_uint32),
        ("n_resident", C.c_uint64), ("n_matched", C.c_uint64), ("error_spans", C.c_uint64),
        ("key_hash", u64p), ("errors", u64p),
    ]


SA_MOVERS_FALL = 1
i64p = C.POINTER(C.c_int64)


class sa_movers_result(C.Structure):
    _fields_ = [
        ("base_first", C.c_uint64), ("base_last", C.c_uint64), ("cur_first", C.c_uint64), ("cur_last", C.c_uint64),
        ("k", C.c_uint32), ("n", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32),
        ("n_resident", C.c_uint64), ("n_matched", C.c_uint64),
        ("error_spans_base", C.c_uint64), ("error_spans_cur", C.c_uint64),
        ("key_hash", u64p), ("score", i64p), ("baseline", u64p), ("current", u64p),
    ]


SA_ERROR_ONSET_FALL = 1


class sa_error_onset_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("k", C.c_uint32), ("n", C.c_uint32),
        ("flags", C.c_uint32), ("pad", C.c_uint32),
        ("n_resident", C.c_uint64), ("n_eligible", C.c_uint64), ("n_matched", C.c_uint64), ("error_spans", C.c_uint64),
        ("key_hash", u64p), ("onset_window", u64p), ("score", i64p), ("errors_before", u64p), ("errors_after", u64p),
    ]


SA_OVERLAP_MAX_SERVICES = OVERLAP_MAX_SERVICES = 64


class sa_overlap_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("n_sel", C.c_uint32), ("n_pairs", C.c_uint32),
        ("hll_p", C.c_uint32), ("pad", C.c_uint32), ("services", u32p), ("hll_hist", u32p), ("distinct", f64p),
        ("pair_hist", u32p), ("union_est", f64p), ("shared", f64p),
    ]


SA_LAT_BINS = LAT_BINS = 256
SA_LAT_MAX_Q = LAT_MAX_Q = 8
SA_LAT_HIST = 1


class sa_latency_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("width", C.c_uint32), ("n_out", C.c_uint32),
        ("n_sel", C.c_uint32), ("n_q", C.c_uint32), ("services", u32p), ("q_ppm", u32p), ("count", u64p),
        ("q_bin", u8p), ("q_ns", u64p), ("hist", u64p),
    ]


SA_LATMOV_FALL = 1
i32p = C.POINTER(C.c_int32)


class sa_latency_movers_result(C.Structure):
    _fields_ = [
        ("base_first", C.c_uint64), ("base_last", C.c_uint64), ("cur_first", C.c_uint64), ("cur_last", C.c_uint64),
        ("k", C.c_uint32), ("n", C.c_uint32), ("n_q", C.c_uint32), ("flags", C.c_uint32),
        ("n_services", C.c_uint64), ("n_eligible", C.c_uint64), ("n_matched", C.c_uint64),
        ("spans_base", C.c_uint64), ("spans_cur", C.c_uint64),
        ("q_ppm", u32p), ("services", u32p), ("shift", i32p), ("count_base", u64p), ("count_cur", u64p),
        ("q_bin_base", u8p), ("q_bin_cur", u8p), ("q_ns_base", u64p), ("q_ns_cur", u64p),
    ]


SA_SLO_MAX_WIDTHS = SLO_MAX_WIDTHS = 4


class sa_slo_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("n_out", C.c_uint32), ("n_sel", C.c_uint32),
        ("n_widths", C.c_uint32), ("pad", C.c_uint32), ("min_count", C.c_uint64),
        ("services", u32p), ("widths", u32p), ("limit_ppm", u32p), ("threshold_ns", u64p), ("threshold_bin", u8p),
        ("effective_ns", u64p), ("total", u64p), ("slow", u64p), ("burning", u8p), ("alert_outputs", u32p),
    ]


SA_ONSET_FALL = 1


class sa_onset_result(C.Structure):
    _fields_ = [
        ("first_window", C.c_uint64), ("last_window", C.c_uint64), ("k", C.c_uint32), ("n", C.c_uint32),
        ("flags", C.c_uint32), ("q_ppm", C.c_uint32), ("min_count", C.c_uint64),
        ("n_services", C.c_uint64), ("n_eligible", C.c_uint64), ("n_matched", C.c_uint64), ("spans", C.c_uint64),
        ("services", u32p), ("onset_window", u64p), ("delta_ppm", i32p), ("threshold_bin", u8p), ("effective_ns", u64p),
        ("total_before", u64p), ("slow_before", u64p), ("total_after", u64p), ("slow_after", u64p),
    ]


class sa_stats(C.Structure):
    _fields_ = [
        ("spans", C.c_uint64), ("zero_key", C.c_uint64), ("invalid_service", C.c_uint64),
        ("window_out_of_range", C.c_uint64), ("dropped_table_full", C.c_uint64),
        ("n_keys", C.c_uint64), ("table_capacity", C.c_uint64), ("window_base", C.c_uint64),
        ("small_table", C.c_uint32), ("pad", C.c_uint32), ("hll_filtered", C.c_uint64),
    ]


class sa_debug_geometry_info(C.Structure):
    """include/spanagg_diag.h: the geometry decisions sa_create took."""
    _fields_ = [
        ("path", C.c_uint32), ("kernel", C.c_uint32), ("block", C.c_uint32), ("grid_max", C.c_uint32),
        ("log2cap", C.c_uint32), ("lb_shift", C.c_uint32), ("lb_n", C.c_uint32), ("error_table", C.c_uint32),
        ("lds_bytes", C.c_uint64),
        ("expo_count", C.c_uint32), ("expo_entries", C.c_uint32), ("expo_bin_slots", C.c_uint32),
        ("expo_bins", C.c_uint32),
    ]


# SA_EXPO_COUNT_* (include/spanagg_diag.h): an exponential engine's counting pass
EXPO_COUNT_NONE, EXPO_COUNT_SLAB, EXPO_COUNT_CACHED, EXPO_COUNT_HBM = 0, 1, 2, 3
PATH_NAMES = ("Small", "ExpoSmall", "ExpoHbm", "Binned", "Dense", "Partitioned", "Atomic")  # sa::Path
# SA_KERNEL_* (include/spanagg_diag.h)
KERNEL_NAMES = ("small_default", "small_512", "small_1024", "small_linear", "expo_specialised", "expo_generic",
                "bounds16", "bounds_generic", "lab")

# (name, restype, argtypes) for every entry point declared in include/spanagg.h
SIGNATURES = [
    ("sa_config_default", None, [C.POINTER(sa_config)]),
    ("sa_abi_version", C.c_int, []),
    ("sa_create", C.c_int, [C.POINTER(sa_config), C.POINTER(C.c_void_p)]),
    ("sa_destroy", None, [C.c_void_p]),
    ("sa_last_error", C.c_char_p, [C.c_void_p]),
    ("sa_ingest", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch)]),
    ("sa_ingest_async", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch)]),
    ("sa_ingest_device", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch), C.c_void_p]),
    ("sa_ingest_device_many", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch), C.c_uint32, C.c_void_p]),
    ("sa_host_alloc", C.c_int, [C.c_size_t, C.POINTER(C.c_void_p)]),
    ("sa_host_free", None, [C.c_void_p]),
    ("sa_sync", C.c_int, [C.c_void_p]),
    ("sa_flush", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(sa_red_result))]),
    ("sa_red_result_free", None, [C.POINTER(sa_red_result)]),
    ("sa_flush_exp", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(sa_exp_result))]),
    ("sa_reclaim_keys", C.c_int, [C.c_void_p, C.c_int]),
    ("sa_exp_result_free", None, [C.POINTER(sa_exp_result)]),
    ("sa_expo_probe", C.c_int, [C.c_void_p, f64p, C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_int32), f64p]),
    ("sa_key_union_probe", C.c_int, [C.c_void_p, u64p, C.c_uint64, u64p, u64p]),
    ("sa_join", C.c_int, [C.c_void_p, C.c_void_p]),
    ("sa_expo_fast_probe", C.c_int, [C.c_void_p, u64p, C.POINTER(C.c_int32), C.c_uint64, C.POINTER(C.c_int32),
                                     C.POINTER(C.c_int32), f64p]),
    ("sa_window_read", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.POINTER(sa_sketch_result))]),
    ("sa_window_advance", C.c_int, [C.c_void_p, C.c_uint64]),
    ("sa_sketch_result_free", None, [C.POINTER(sa_sketch_result)]),
    ("sa_window_range", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u64p, C.c_uint64, C.c_uint32,
                                  C.POINTER(C.POINTER(sa_range_result))]),
    ("sa_group_window_range", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u64p, C.c_uint64, C.c_uint32,
                                        C.POINTER(C.POINTER(sa_range_result))]),
    ("sa_range_result_free", None, [C.POINTER(sa_range_result)]),
    ("sa_window_series", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, u64p, C.c_uint64, C.c_uint32,
                                   C.POINTER(C.POINTER(sa_series_result))]),
    ("sa_series_result_free", None, [C.POINTER(sa_series_result)]),
    ("sa_window_top", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                C.POINTER(C.POINTER(sa_top_result))]),
    ("sa_group_window_top", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32,
                                      C.POINTER(C.POINTER(sa_top_result))]),
    ("sa_top_result_free", None, [C.POINTER(sa_top_result)]),
    ("sa_window_movers", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64,
                                   C.c_uint32, C.POINTER(C.POINTER(sa_movers_result))]),
    ("sa_group_window_movers", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                         C.c_uint64, C.c_uint32, C.POINTER(C.POINTER(sa_movers_result))]),
    ("sa_movers_result_free", None, [C.POINTER(sa_movers_result)]),
    ("sa_window_error_onset", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                        C.c_uint32, C.POINTER(C.POINTER(sa_error_onset_result))]),
    ("sa_group_window_error_onset", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64,
                                              C.c_uint32, C.POINTER(C.POINTER(sa_error_onset_result))]),
    ("sa_error_onset_result_free", None, [C.POINTER(sa_error_onset_result)]),
    ("sa_window_overlap", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u32p, C.c_uint32, C.c_uint32,
                                    C.POINTER(C.POINTER(sa_overlap_result))]),
    ("sa_group_window_overlap", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u32p, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.POINTER(sa_overlap_result))]),
    ("sa_overlap_result_free", None, [C.POINTER(sa_overlap_result)]),
    ("sa_window_latency", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32,
                                    C.c_uint32, C.POINTER(C.POINTER(sa_latency_result))]),
    ("sa_group_window_latency", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, u32p, C.c_uint32, u32p,
                                          C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(sa_latency_result))]),
    ("sa_latency_result_free", None, [C.POINTER(sa_latency_result)]),
    ("sa_window_latency_movers", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                           C.c_uint64, C.c_uint32, u32p, C.c_uint32, C.c_uint32,
                                           C.POINTER(C.POINTER(sa_latency_movers_result))]),
    ("sa_group_window_latency_movers", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                                 C.c_uint32, C.c_uint64, C.c_uint32, u32p, C.c_uint32, C.c_uint32,
                                                 C.POINTER(C.POINTER(sa_latency_movers_result))]),
    ("sa_latency_movers_result_free", None, [C.POINTER(sa_latency_movers_result)]),
    ("sa_window_slo", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint32, u32p, C.c_uint32, u64p,
                                C.c_uint64, C.c_uint32, C.POINTER(C.POINTER(sa_slo_result))]),
    ("sa_group_window_slo", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, u32p, u32p, C.c_uint32, u32p, C.c_uint32,
                                      u64p, C.c_uint64, C.c_uint32, C.POINTER(C.POINTER(sa_slo_result))]),
    ("sa_slo_result_free", None, [C.POINTER(sa_slo_result)]),
    ("sa_window_latency_onset", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u64p, C.c_uint64,
                                          C.c_uint32, C.c_uint32, C.POINTER(C.POINTER(sa_onset_result))]),
    ("sa_group_window_latency_onset", C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, u64p,
                                                C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.POINTER(C.POINTER(sa_onset_result))]),
    ("sa_onset_result_free", None, [C.POINTER(sa_onset_result)]),
    ("sa_onset_probe", C.c_int, [C.c_void_p, u64p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                 C.c_uint32, C.POINTER(C.POINTER(sa_onset_result))]),
    ("sa_latency_bin", C.c_uint32, [C.c_uint64]),
    ("sa_latency_bin_bounds", C.c_int, [C.c_uint32, u64p, u64p]),
    ("sa_hll_estimate_hist", C.c_double, [u32p, C.c_uint32]),
    ("sa_get_stats", C.c_int, [C.c_void_p, C.POINTER(sa_stats)]),
    ("sa_bind_ids", C.c_int, [C.c_void_p, u64p, u64p, C.c_uint64]),
    ("sa_export_keys", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, u64p, C.c_void_p]),
    ("sa_gather_dense", C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_int, C.c_void_p]),
    ("sa_window_export", C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("sa_group_create", C.c_int, [C.POINTER(sa_config), C.POINTER(C.c_int32), C.c_uint32,
                                  C.POINTER(C.c_void_p)]),
    ("sa_group_destroy", None, [C.c_void_p]),
    ("sa_group_last_error", C.c_char_p, [C.c_void_p]),
    ("sa_group_size", C.c_uint32, [C.c_void_p]),
    ("sa_group_uses_rccl", C.c_int, [C.c_void_p]),
    ("sa_group_member", C.c_void_p, [C.c_void_p, C.c_uint32]),
    ("sa_group_ingest", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch)]),
    ("sa_group_ingest_device", C.c_int, [C.c_void_p, C.POINTER(sa_span_batch), C.c_uint32, C.c_void_p]),
    ("sa_group_sync", C.c_int, [C.c_void_p]),
    ("sa_group_flush", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(sa_red_result))]),
    ("sa_group_flush_exp", C.c_int, [C.c_void_p, C.POINTER(C.POINTER(sa_exp_result))]),
    ("sa_group_window_read", C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.POINTER(sa_sketch_result))]),
    ("sa_group_window_advance", C.c_int, [C.c_void_p, C.c_uint64]),
    ("sa_group_get_stats", C.c_int, [C.c_void_p, C.POINTER(sa_stats)]),
    ("sa_debug_stamps", C.c_int, [C.c_void_p, u64p, C.c_uint64, u64p]),
    ("sa_debug_geometry", C.c_int, [C.c_void_p, C.POINTER(sa_debug_geometry_info)]),
    ("sa_bucket_thresholds", C.c_int, [f64p, C.c_uint32, C.c_uint32, u64p, u32p]),
    ("sa_hll_estimate", C.c_double, [u8p, C.c_uint32]),
]

ABI_VERSION = 4  # include/spanagg.h SA_ABI_VERSION

_lib = None


def load() -> C.CDLL:
    """Load libspanagg.so (in-tree build). Raises if it was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"libspanagg.so not found at {LIB_PATH}; build it with "
                "`make -C opentelemetry-demo_amd` (or __graft_entry__.build())")
        # torch ships its own libamdhip64.so.7. Loading torch first makes
        # libspanagg bind to that same HIP runtime (same soname), so device
        # pointers and streams are shared; loading /opt/rocm's copy first
        # leaves torch with a second runtime that sees no GPUs.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = C.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES:
            fn = getattr(lib, name, None)
            if fn is None and os.environ.get("SPANAGG_LIB"):
                continue  # an older diagnostic build may lack newer entry points
            if fn is None:
                raise RuntimeError(f"libspanagg.so does not export {name}")
            fn.restype = res
            fn.argtypes = args
        if lib.sa_abi_version() != ABI_VERSION:
            raise RuntimeError("libspanagg ABI version mismatch")
        _lib = lib
    return _lib


class SpanAggError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(code, code)}: {msg}")
        self.code = code
