"""spanagg -- host side of the MI355X span-aggregation engine.

The hot path (per-span RED aggregation + HLL / count-min sketches) runs in
libspanagg.so's HIP kernels; this package binds its C-ABI, builds and hashes
dimension keys, generates synthetic workloads and merges partials across
ranks.  Importing it does not require a GPU; creating an Engine does.
"""
from .engine import (DEFAULT_BOUNDS_MS, Config, Engine, ErrorOnsetResult, Group, LatencyMoversResult, LatencyResult, MoversResult,
                     OnsetResult, OverlapResult, RangeResult, RedResult, SeriesResult, SketchResult, SloResult, SpanBatch, TopResult,
                     bucket_thresholds, hll_estimate, hll_estimate_hist, pack_meta, trace_words)
from ._lib import (LAT_BINS, LAT_MAX_Q, OVERLAP_MAX_SERVICES, SA_ERROR_ONSET_FALL, SA_LATMOV_FALL, SA_MOVERS_FALL, SA_ONSET_FALL, SLO_MAX_WIDTHS,
                   TOP_MAX_K,
                   SpanAggError, load)
from .dense import DenseIds

__all__ = [
    "DEFAULT_BOUNDS_MS", "Config", "DenseIds", "Engine", "ErrorOnsetResult", "Group", "LAT_BINS", "LAT_MAX_Q", "LatencyMoversResult",
    "LatencyResult", "MoversResult", "OVERLAP_MAX_SERVICES", "OnsetResult", "OverlapResult",
    "RangeResult", "RedResult", "SA_ERROR_ONSET_FALL", "SA_LATMOV_FALL", "SA_MOVERS_FALL", "SA_ONSET_FALL", "SLO_MAX_WIDTHS", "SeriesResult",
    "SketchResult", "SloResult", "SpanBatch", "SpanAggError", "TOP_MAX_K", "TopResult", "bucket_thresholds", "hll_estimate", "hll_estimate_hist", "load", "pack_meta",
    "trace_words",
]
