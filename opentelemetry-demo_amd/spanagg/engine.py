"""Python host wrapper of one libspanagg engine (one engine per GPU / rank).

Maps the connector's lifecycle onto the C-ABI:
``Engine(config)`` ~ createTracesToMetricsConnector + Start, ``ingest`` ~ the
per-span body of ConsumeTraces, ``flush`` ~ exportMetrics' buildMetrics +
resetState (delta since the previous flush), ``close`` ~ Shutdown.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import SpanAggError
from .dense import DenseIds

DEFAULT_BOUNDS_MS = (2, 4, 6, 8, 10, 50, 100, 200, 400, 800, 1000, 1400, 2000, 5000, 10000, 15000)

KIND_SHIFT, STATUS_SHIFT = 16, 19


def pack_meta(service_id, kind, status) -> np.ndarray:
    """meta = service_id | kind << 16 | status << 19 (SoA v1)."""
    s = np.asarray(service_id, dtype=np.uint32)
    k = np.asarray(kind, dtype=np.uint32)
    c = np.asarray(status, dtype=np.uint32)
    if np.any(s > 0xFFFF) or np.any(k > 7) or np.any(c > 3):
        raise ValueError("meta field out of range")
    return (s | (k << KIND_SHIFT) | (c << STATUS_SHIFT)).astype(np.uint32)


def trace_words(trace_ids: np.ndarray):
    """[n,16] u8 wire trace ids -> (w0, w1) little-endian u64 words."""
    t = np.ascontiguousarray(trace_ids, dtype=np.uint8).reshape(-1, 16)
    w = t.view("<u8").reshape(-1, 2)
    return np.ascontiguousarray(w[:, 0]), np.ascontiguousarray(w[:, 1])


@dataclass
class Config:
    """Mirror of the spanmetrics Config fields this engine consumes plus the
    build-owned sketch parameters (defaults = the reference's empty
    `spanmetrics:` block, otelcol-config.yml:115-116)."""
    bounds: Sequence[float] = DEFAULT_BOUNDS_MS
    unit: str = "ms"
    hll_p: int = 14
    cms_d: int = 4
    cms_w: int = 2048
    window_ns: int = 10_000_000_000
    n_windows: int = 8
    n_services: int = 64
    key_capacity: int = 1000
    device: int = 0
    flags: int = 0  # SA_DIAG_* profiling ablations only (laboratory build; results are wrong when set)
    exp_max_size: int = 0  # histogram.exponential.max_size (0: explicit buckets)
    options: int = 0  # SA_OPT_* path options (spanagg._lib.OPT_*): same results, another kernel path

    def to_c(self):
        arr = (C.c_double * max(1, len(self.bounds)))(*[float(b) for b in self.bounds])
        c = _lib.sa_config()
        c.bounds = C.cast(arr, _lib.f64p)
        c.n_bounds = len(self.bounds)
        c.unit = _lib.SA_UNIT_S if self.unit == "s" else _lib.SA_UNIT_MS
        c.hll_p, c.cms_d, c.cms_w = self.hll_p, self.cms_d, self.cms_w
        c.window_ns, c.n_windows, c.n_services = self.window_ns, self.n_windows, self.n_services
        c.key_capacity, c.device, c.flags = self.key_capacity, self.device, self.flags
        c.exp_max_size, c.options = self.exp_max_size, self.options
        return c, arr


@dataclass
class SpanBatch:
    key_hash: np.ndarray
    start_ns: np.ndarray
    end_ns: np.ndarray
    trace_w0: np.ndarray
    trace_w1: np.ndarray
    meta: np.ndarray

    def __post_init__(self):
        for name in ("key_hash", "start_ns", "end_ns", "trace_w0", "trace_w1"):
            setattr(self, name, np.ascontiguousarray(getattr(self, name), dtype=np.uint64))
        self.meta = np.ascontiguousarray(self.meta, dtype=np.uint32)
        n = len(self.key_hash)
        if any(len(getattr(self, f)) != n for f in
               ("start_ns", "end_ns", "trace_w0", "trace_w1", "meta")):
            raise ValueError("ragged SoA batch")

    def __len__(self):
        return len(self.key_hash)

    def slice(self, a: int, b: int) -> "SpanBatch":
        return SpanBatch(self.key_hash[a:b], self.start_ns[a:b], self.end_ns[a:b],
                         self.trace_w0[a:b], self.trace_w1[a:b], self.meta[a:b])

    def columns(self):
        return (self.key_hash, self.start_ns, self.end_ns, self.trace_w0, self.trace_w1, self.meta)


@dataclass
class RedResult:
    key_hash: np.ndarray          # [n] u64, ascending
    bucket_counts: np.ndarray     # [n, n_buckets] u64
    calls: np.ndarray             # [n] u64
    sum_ns: np.ndarray            # [n] u64
    sum: np.ndarray               # [n] f64 (ms or s)
    status: int = 0


@dataclass
class ExpoResult:
    """sa_exp_result: per series go-expohisto histograms (delta since the last flush)."""
    key_hash: np.ndarray     # [n] u64, ascending
    count: np.ndarray        # [n] u64
    zero_count: np.ndarray   # [n] u64
    sum_ns: np.ndarray       # [n] u64
    sum: np.ndarray          # [n] f64 (unit)
    min: np.ndarray
    max: np.ndarray
    scale: np.ndarray        # [n] i32
    offset: np.ndarray       # [n] i32
    buckets: list            # [n] u64 arrays (positive buckets offset .. offset + len - 1)
    status: int = 0


@dataclass
class SketchResult:
    window_id: int
    hll: np.ndarray               # [n_services, 2^p] u8
    cms: np.ndarray               # [d, w] u32
    p: int = 14

    def distinct_traces(self, service_id: int) -> float:
        return hll_estimate(self.hll[service_id], self.p)


@dataclass
class RangeResult:
    """sa_range_result: the sketches of windows first..last merged on the device."""
    first: int
    last: int
    hist: np.ndarray              # [n_services, 64] u32: merged registers holding each value
    distinct: np.ndarray          # [n_services] f64: hll_estimate_hist(hist[s], p)
    hll: Optional[np.ndarray]     # [n_services, 2^p] u8 merged registers (registers=True), else None
    cms: Optional[np.ndarray]     # [d, w] u64 summed cells, unsaturated (cells=True), else None
    errors: np.ndarray            # [n_keys] u64: the merged count-min's estimate for keys[i]
    keys: np.ndarray              # [n_keys] u64, as given
    p: int = 14

    def top_errors(self, k: int = 10):
        """Top-k (key, estimate) of the queried keys, ordered as sketch.heavy_hitters."""
        est = [(int(key), int(e)) for key, e in zip(self.keys, self.errors) if e > 0]
        est.sort(key=lambda e: (-e[1], e[0]))
        return est[:k]


@dataclass
class SeriesResult:
    """sa_series_result: row i is window first + i's answer over the trailing
    `width` windows (what window_range(first + i - width + 1, first + i, keys) returns)."""
    first: int
    last: int
    width: int
    hist: np.ndarray              # [n_out, n_services, 64] u32
    distinct: np.ndarray          # [n_out, n_services] f64: hll_estimate_hist(hist[i, s], p)
    error_spans: np.ndarray       # [n_out] u64: ERROR spans the covered windows' sketches counted, exact
    errors: np.ndarray            # [n_out, n_keys] u64: the summed count-min's estimate for keys[j]
    keys: np.ndarray              # [n_keys] u64, as given
    p: int = 14

    def top_errors(self, i: int, k: int = 10):
        """Row i's top-k (key, estimate) of the queried keys, ordered as sketch.heavy_hitters."""
        est = [(int(key), int(e)) for key, e in zip(self.keys, self.errors[i]) if e > 0]
        est.sort(key=lambda e: (-e[1], e[0]))
        return est[:k]


@dataclass
class TopResult:
    """sa_top_result: the heaviest ERROR series of windows first..last among the
    series resident in the engine's key table, by the summed count-min."""
    first: int
    last: int
    keys: np.ndarray              # [n] u64, by estimate descending then key ascending
    errors: np.ndarray            # [n] u64: window_range(first, last, [keys[i]]).errors[0]
    n_resident: int               # series in the key table when the call ran: the candidates
    n_matched: int                # candidates with an estimate >= min_count
    error_spans: int              # ERROR spans the range's sketches counted, exact

    def items(self):
        """[(key, estimate)] as sketch.heavy_hitters returns them."""
        return [(int(k), int(e)) for k, e in zip(self.keys, self.errors)]


@dataclass
class MoversResult:
    """sa_movers_result: the series whose ERROR spans per window rose most (fall:
    fell most) from the baseline range to the current one, among the series
    resident in the engine's key table, by the two ranges' summed count-mins."""
    base: tuple                   # (first, last) of the baseline range
    cur: tuple                    # (first, last) of the current range
    fall: bool
    keys: np.ndarray              # [n] u64, by score descending then key ascending
    score: np.ndarray             # [n] i64: current * n_base - baseline * n_cur (negated when fall), >= 1
    baseline: np.ndarray          # [n] u64: window_range(*base, [keys[i]]).errors[0]
    current: np.ndarray           # [n] u64: window_range(*cur, [keys[i]]).errors[0]
    n_resident: int               # series in the key table when the call ran: the candidates
    n_matched: int                # candidates with a score >= max(min_score, 1)
    error_spans_base: int         # ERROR spans the baseline range's sketches counted, exact
    error_spans_cur: int          # the same of the current range

    def items(self):
        """[(key, score, baseline, current)] as sketch.movers returns them."""
        return [(int(k), int(s), int(b), int(c)) for k, s, b, c in zip(self.keys, self.score, self.baseline, self.current)]


@dataclass
class ErrorOnsetResult:
    """sa_error_onset_result: the series whose ERROR spans per window rose most
    (fall: fell most) across their best split of windows first..last, among the
    series resident in the engine's key table -- each with the window at which
    "after" begins."""
    first_window: int
    last_window: int
    fall: bool
    keys: np.ndarray              # [n] u64, by score descending then key ascending
    onset_window: np.ndarray      # [n] u64: the first window of "after"
    score: np.ndarray             # [n] i64: after * t - before * (n - t) at the best split (negated when fall), >= 1
    errors_before: np.ndarray     # [n] u64: window_range(first, onset_window - 1, [keys[i]]).errors[0]
    errors_after: np.ndarray      # [n] u64: window_range(onset_window, last, [keys[i]]).errors[0]
    n_resident: int               # series in the key table when the call ran: the candidates
    n_eligible: int               # candidates with an estimate over the range >= max(min_count, 1)
    n_matched: int                # eligible candidates with a best score >= max(min_score, 1)
    error_spans: int              # ERROR spans the range's sketches counted, exact

    def items(self):
        """[(key, onset_window, score, errors_before, errors_after)]; sketch.error_onset's rows with t = onset_window - first."""
        return [tuple(int(v) for v in row) for row in zip(self.keys, self.onset_window, self.score, self.errors_before,
                                                          self.errors_after)]


@dataclass
class OverlapResult:
    """sa_overlap_result: for every pair of the selected services the traces
    both saw over windows first..last, by inclusion-exclusion on the merged
    HyperLogLog registers (the register-wise maximum of two services' arrays is
    the sketch of the union of their trace sets).  Each estimate carries about
    1.04 / sqrt(2^p) relative error of its own size: `shared` means something
    only where it is not small against union x 1.04 / sqrt(2^p)."""
    first: int
    last: int
    services: np.ndarray          # [n] u32 service ids, in the caller's order
    hist: np.ndarray              # [n, 64] u32: window_range(first, last).hist[services]
    distinct: np.ndarray          # [n] f64: window_range(first, last).distinct[services]
    pair_hist: np.ndarray         # [n_pairs, 64] u32: histogram of max(regs[i], regs[j]), row pair_index(i, j)
    union: np.ndarray             # [n, n] f64, symmetric, diagonal = distinct
    shared: np.ndarray            # [n, n] f64, symmetric, diagonal = distinct
    p: int = 14

    def pair_index(self, i: int, j: int) -> int:
        """Row of pair_hist for positions i != j of `services`."""
        n = len(self.services)
        i, j = (i, j) if i < j else (j, i)
        if not 0 <= i < j < n:
            raise IndexError("pair_index: two different positions of the selection")
        return i * n - i * (i + 1) // 2 + (j - i - 1)

    def strongest(self, k: int = 10):
        """The k pairs with the largest `shared`, ties by (i, j):
        [(services[i], services[j], shared)] with i < j."""
        n = len(self.services)
        pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
        pairs.sort(key=lambda ij: (-float(self.shared[ij]), ij))
        return [(int(self.services[i]), int(self.services[j]), float(self.shared[i, j])) for i, j in pairs[:k]]


@dataclass
class LatencyResult:
    """sa_latency_result: per output window and selected service the spans of
    the covered windows and, for each quantile, the histogram bin that holds it
    and that bin's upper bound in ns -- an upper bound on the true quantile,
    within 12.5 % (127 ns below 2,048 ns)."""
    first: int
    last: int
    width: int
    services: np.ndarray          # [n_sel] u32 service ids, in the caller's order
    q_ppm: np.ndarray             # [n_q] u32: round(quantile * 1e6)
    count: np.ndarray             # [n_out, n_sel] u64
    q_bin: np.ndarray             # [n_out, n_sel, n_q] u8
    q_ns: np.ndarray              # [n_out, n_sel, n_q] u64: sketch.latency_bin_bounds(q_bin)[1]; 0 where count == 0
    hist: Optional[np.ndarray]    # [n_out, n_sel, 256] u64 summed bins (hist=True), else None


@dataclass
class LatencyMoversResult:
    """sa_latency_movers_result: the services whose ranking quantile (q_ppm[0])
    moved up most bins (fall: down) from the baseline range's summed histogram
    to the current range's, among the services with enough spans in both.
    From 2,048 ns up eight bins are a factor of two."""
    base: tuple                   # (first, last) of the baseline range
    cur: tuple                    # (first, last) of the current range
    fall: bool
    q_ppm: np.ndarray             # [n_q] u32: round(quantile * 1e6); q_ppm[0] ranks
    services: np.ndarray          # [n] u32, by shift descending, count_cur descending, id ascending
    shift: np.ndarray             # [n] i32: q_bin_cur[:, 0] - q_bin_base[:, 0] (negated when fall), >= 1
    count_base: np.ndarray        # [n] u64: window_latency(*base, services=[s]).count
    count_cur: np.ndarray         # [n] u64
    q_bin_base: np.ndarray        # [n, n_q] u8: window_latency(*base, services=[s], quantiles).q_bin
    q_bin_cur: np.ndarray         # [n, n_q] u8
    q_ns_base: np.ndarray         # [n, n_q] u64: the bins' upper bounds in ns
    q_ns_cur: np.ndarray          # [n, n_q] u64
    n_services: int               # the candidates: every service
    n_eligible: int               # services with at least max(min_count, 1) spans in both ranges
    n_matched: int                # eligible services with shift >= max(min_shift, 1)
    spans_base: int               # spans of every service over the baseline range, exact
    spans_cur: int                # the same of the current range

    def items(self):
        """[(service, shift, count_base, count_cur, q_bin_base, q_bin_cur)] as sketch.latency_movers returns them."""
        return [(int(s), int(d), int(b), int(c), tuple(int(x) for x in qb), tuple(int(x) for x in qc))
                for s, d, b, c, qb, qc in zip(self.services, self.shift, self.count_base, self.count_cur,
                                              self.q_bin_base, self.q_bin_cur)]


@dataclass
class SloResult:
    """sa_slo_result: per output window, width and selected service the spans
    of the covered windows and those slower than the service's threshold, and
    whether each width burns its error budget -- slow * 10^6 > limit_ppm *
    total with at least min_count spans.  "Slow" means a duration above
    effective_ns, the upper bound of the threshold's histogram bin."""
    first: int
    last: int
    min_count: int                # as applied: max(min_count, 1)
    services: np.ndarray          # [n_sel] u32 service ids, in the caller's order
    widths: np.ndarray            # [n_widths] u32 as given
    limit_ppm: np.ndarray         # [n_widths] u32 as given
    threshold_ns: np.ndarray      # [n_sel] u64 as given
    threshold_bin: np.ndarray     # [n_sel] u8: sketch.latency_bin(threshold_ns)
    effective_ns: np.ndarray      # [n_sel] u64: sketch.latency_bin_bounds(threshold_bin)[1]
    total: np.ndarray             # [n_out, n_widths, n_sel] u64
    slow: np.ndarray              # [n_out, n_widths, n_sel] u64
    burning: np.ndarray           # [n_out, n_sel] u8: bit w set when width w burns
    alert_outputs: np.ndarray     # [n_sel] u32: outputs at which every width burns


@dataclass
class OnsetResult:
    """sa_onset_result: the services whose share of slow spans changed most
    inside first..last, each with the window at which "after" begins.  A span is
    slow above its service's threshold bin -- the given threshold's, or the bin
    of the pooled quantile q_ppm of the service's spans over the whole range."""
    first: int
    last: int
    fall: bool
    q_ppm: int                    # as given; 0 when thresholds were given
    min_count: int                # as applied: max(min_count, 1)
    services: np.ndarray          # [n] u32, by delta_ppm descending, spans descending, id ascending
    onset_window: np.ndarray      # [n] u64: the first window of "after"
    delta_ppm: np.ndarray         # [n] i32: the slow share after minus before in ppm (negated when fall), >= 1
    threshold_bin: np.ndarray     # [n] u8
    effective_ns: np.ndarray      # [n] u64: sketch.latency_bin_bounds(threshold_bin)[1]
    total_before: np.ndarray      # [n] u64: spans of first .. onset_window - 1
    slow_before: np.ndarray       # [n] u64
    total_after: np.ndarray       # [n] u64: spans of onset_window .. last
    slow_after: np.ndarray        # [n] u64
    n_services: int               # the candidates: every service
    n_eligible: int               # services with a split that leaves max(min_count, 1) spans on both sides
    n_matched: int                # eligible services whose slow share changed by at least max(min_delta_ppm, 1)
    spans: int                    # spans of every service over the range, exact

    def items(self):
        """[(service, onset_window, delta_ppm, total_before, slow_before, total_after, slow_after)]."""
        return [tuple(int(v) for v in row) for row in zip(self.services, self.onset_window, self.delta_ppm,
                                                          self.total_before, self.slow_before, self.total_after,
                                                          self.slow_after)]


def hll_estimate(regs: np.ndarray, p: int) -> float:
    lib = _lib.load()
    r = np.ascontiguousarray(regs, dtype=np.uint8)
    return float(lib.sa_hll_estimate(r.ctypes.data_as(_lib.u8p), p))


def hll_estimate_hist(hist: np.ndarray, p: int) -> float:
    """sa_hll_estimate_hist: the estimate from a register array's value
    histogram (64 counts), exact in the sum and so independent of its order."""
    lib = _lib.load()
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    if h.shape != (_lib.SA_HLL_HIST_BINS,):
        raise ValueError("hll_estimate_hist: the histogram has 64 bins")
    return float(lib.sa_hll_estimate_hist(h.ctypes.data_as(_lib.u32p), p))


def bucket_thresholds(bounds, unit: str = "ms"):
    lib = _lib.load()
    b = np.ascontiguousarray(bounds, dtype=np.float64)
    thr = np.zeros(max(1, len(b)), dtype=np.uint64)
    nneg = C.c_uint32(0)
    rc = lib.sa_bucket_thresholds(b.ctypes.data_as(_lib.f64p), len(b),
                                  _lib.SA_UNIT_S if unit == "s" else _lib.SA_UNIT_MS,
                                  thr.ctypes.data_as(_lib.u64p), C.byref(nneg))
    if rc != 0:
        raise SpanAggError(rc, "invalid histogram bounds")
    return thr[: len(b) - nneg.value], nneg.value


class _ResultOwner:
    """Frees an sa_red_result once the last numpy view of its columns is gone."""

    def __init__(self, lib, out):
        self.lib, self.out = lib, out

    def __del__(self):
        self.lib.sa_red_result_free(self.out)


def _red_result(owner, rc: int, out, allow_drops: bool, what: str, _fn=None) -> RedResult:
    """numpy views of an sa_red_result's columns (no copy: a C4-scale flush is
    ~170 MB); the result is freed when the last view is collected."""
    lib = owner.lib
    if rc not in (0, _lib.SA_EFULL) or not out:
        owner._check(rc if rc else _lib.SA_ESTATE, what)
    keep = _ResultOwner(lib, out)
    r = out.contents
    n, nb = int(r.n_series), int(r.n_buckets)

    def arr(p, shape, dt):
        if n == 0:
            return np.zeros(shape, dtype=dt)
        count = int(np.prod(shape))
        buf = (C.c_uint64 * count).from_address(C.cast(p, C.c_void_p).value)
        buf._keep = keep  # the views' base holds the result
        return np.frombuffer(buf, dtype=dt).reshape(shape)

    res = RedResult(arr(r.key_hash, (n,), np.uint64), arr(r.bucket_counts, (n, nb), np.uint64),
                    arr(r.calls, (n,), np.uint64), arr(r.sum_ns, (n,), np.uint64),
                    arr(r.sum, (n,), np.float64), rc)
    del keep
    if rc == _lib.SA_EFULL and not allow_drops:
        raise SpanAggError(rc, f"{what}: spans dropped (key table full); stats={owner.stats()}")
    return res


def _sketch_result(lib, out) -> SketchResult:
    try:
        r = out.contents
        hll = np.ctypeslib.as_array(r.hll, shape=(r.n_services, 1 << r.hll_p)).copy()
        cms = np.ctypeslib.as_array(r.cms, shape=(r.cms_d, r.cms_w)).copy()
        return SketchResult(int(r.window_id), hll, cms, int(r.hll_p))
    finally:
        lib.sa_sketch_result_free(out)


def _window_range(obj, fn, what, first, last, keys, registers, cells) -> RangeResult:
    """sa_window_range / sa_group_window_range -> RangeResult (copies), freeing the library's result."""
    k = np.ascontiguousarray(() if keys is None else keys, dtype=np.uint64).reshape(-1)
    flags = (_lib.SA_RANGE_REGISTERS if registers else 0) | (_lib.SA_RANGE_CELLS if cells else 0)
    out = C.POINTER(_lib.sa_range_result)()
    obj._check(fn(obj._h, int(first), int(last), k.ctypes.data_as(_lib.u64p) if len(k) else None, len(k), flags,
                  C.byref(out)), what)
    try:
        r = out.contents
        S, p = int(r.n_services), int(r.hll_p)
        return RangeResult(
            int(r.first_window), int(r.last_window),
            np.ctypeslib.as_array(r.hll_hist, shape=(S, _lib.SA_HLL_HIST_BINS)).copy(),
            np.ctypeslib.as_array(r.distinct, shape=(S,)).copy(),
            np.ctypeslib.as_array(r.hll, shape=(S, 1 << p)).copy() if r.hll else None,
            np.ctypeslib.as_array(r.cms, shape=(r.cms_d, r.cms_w)).copy() if r.cms else None,
            np.ctypeslib.as_array(r.errors, shape=(len(k),)).copy() if len(k) else np.zeros(0, np.uint64),
            k, p)
    finally:
        obj.lib.sa_range_result_free(out)


def _window_top(obj, fn, what, first, last, k, min_count) -> TopResult:
    """sa_window_top / sa_group_window_top -> TopResult (copies), freeing the library's result."""
    out = C.POINTER(_lib.sa_top_result)()
    obj._check(fn(obj._h, int(first), int(last), int(k), int(min_count), 0, C.byref(out)), what)
    try:
        r = out.contents
        n = int(r.n)
        col = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.uint64)
        return TopResult(int(r.first_window), int(r.last_window), col(r.key_hash), col(r.errors),
                         int(r.n_resident), int(r.n_matched), int(r.error_spans))
    finally:
        obj.lib.sa_top_result_free(out)


def _window_movers(obj, fn, what, base, cur, k, min_score, fall) -> MoversResult:
    """sa_window_movers / sa_group_window_movers -> MoversResult (copies), freeing the library's result."""
    (bf, bl), (cf, cl) = base, cur
    out = C.POINTER(_lib.sa_movers_result)()
    obj._check(fn(obj._h, int(bf), int(bl), int(cf), int(cl), int(k), int(min_score),
                  _lib.SA_MOVERS_FALL if fall else 0, C.byref(out)), what)
    try:
        r = out.contents
        n = int(r.n)
        col = lambda p, dt=np.uint64: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dt)
        return MoversResult((int(r.base_first), int(r.base_last)), (int(r.cur_first), int(r.cur_last)),
                            bool(r.flags & _lib.SA_MOVERS_FALL), col(r.key_hash), col(r.score, np.int64),
                            col(r.baseline), col(r.current), int(r.n_resident), int(r.n_matched),
                            int(r.error_spans_base), int(r.error_spans_cur))
    finally:
        obj.lib.sa_movers_result_free(out)


def _window_error_onset(obj, fn, what, first, last, k, min_count, min_score, fall) -> ErrorOnsetResult:
    """sa_window_error_onset / sa_group_window_error_onset -> ErrorOnsetResult (copies), freeing the library's result."""
    out = C.POINTER(_lib.sa_error_onset_result)()
    obj._check(fn(obj._h, int(first), int(last), int(k), int(min_count), int(min_score),
                  _lib.SA_ERROR_ONSET_FALL if fall else 0, C.byref(out)), what)
    try:
        r = out.contents
        n = int(r.n)
        col = lambda p, dt=np.uint64: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dt)
        return ErrorOnsetResult(int(r.first_window), int(r.last_window), bool(r.flags & _lib.SA_ERROR_ONSET_FALL),
                                col(r.key_hash), col(r.onset_window), col(r.score, np.int64), col(r.errors_before),
                                col(r.errors_after), int(r.n_resident), int(r.n_eligible), int(r.n_matched),
                                int(r.error_spans))
    finally:
        obj.lib.sa_error_onset_result_free(out)


def _window_overlap(obj, fn, what, first, last, services) -> OverlapResult:
    """sa_window_overlap / sa_group_window_overlap -> OverlapResult (copies), freeing the library's result."""
    sv = None if services is None else np.ascontiguousarray(services, dtype=np.uint32).reshape(-1)
    out = C.POINTER(_lib.sa_overlap_result)()
    obj._check(fn(obj._h, int(first), int(last), None if sv is None else sv.ctypes.data_as(_lib.u32p),
                  0 if sv is None else len(sv), 0, C.byref(out)), what)
    try:
        r = out.contents
        n, npairs, B = int(r.n_sel), int(r.n_pairs), _lib.SA_HLL_HIST_BINS
        distinct = np.ctypeslib.as_array(r.distinct, shape=(n,)).copy()
        union, shared = np.diag(distinct), np.diag(distinct)
        if npairs:
            iu = np.triu_indices(n, 1)  # (row-major i < j: the pair index's order)
            for m, col in ((union, r.union_est), (shared, r.shared)):
                m[iu] = np.ctypeslib.as_array(col, shape=(npairs,))
                m.T[iu] = m[iu]
        return OverlapResult(
            int(r.first_window), int(r.last_window), np.ctypeslib.as_array(r.services, shape=(n,)).copy(),
            np.ctypeslib.as_array(r.hll_hist, shape=(n, B)).copy(), distinct,
            np.ctypeslib.as_array(r.pair_hist, shape=(npairs, B)).copy() if npairs else np.zeros((0, B), np.uint32),
            union, shared, int(r.hll_p))
    finally:
        obj.lib.sa_overlap_result_free(out)


def _window_latency(obj, fn, what, first, last, width, services, quantiles, hist) -> LatencyResult:
    """sa_window_latency / sa_group_window_latency -> LatencyResult (copies), freeing the library's result."""
    sv = None if services is None else np.ascontiguousarray(services, dtype=np.uint32).reshape(-1)
    ppm = np.ascontiguousarray([int(round(float(q) * 1e6)) for q in quantiles], dtype=np.uint32)
    out = C.POINTER(_lib.sa_latency_result)()
    obj._check(fn(obj._h, int(first), int(last), int(width), None if sv is None else sv.ctypes.data_as(_lib.u32p),
                  0 if sv is None else len(sv), ppm.ctypes.data_as(_lib.u32p), len(ppm),
                  _lib.SA_LAT_HIST if hist else 0, C.byref(out)), what)
    try:
        r = out.contents
        n, S, Q = int(r.n_out), int(r.n_sel), int(r.n_q)
        return LatencyResult(
            int(r.first_window), int(r.last_window), int(r.width),
            np.ctypeslib.as_array(r.services, shape=(S,)).copy(), np.ctypeslib.as_array(r.q_ppm, shape=(Q,)).copy(),
            np.ctypeslib.as_array(r.count, shape=(n, S)).copy(), np.ctypeslib.as_array(r.q_bin, shape=(n, S, Q)).copy(),
            np.ctypeslib.as_array(r.q_ns, shape=(n, S, Q)).copy(),
            np.ctypeslib.as_array(r.hist, shape=(n, S, _lib.SA_LAT_BINS)).copy() if r.hist else None)
    finally:
        obj.lib.sa_latency_result_free(out)


def _window_latency_movers(obj, fn, what, base, cur, k, quantiles, min_count, min_shift, fall) -> LatencyMoversResult:
    """sa_window_latency_movers / sa_group_window_latency_movers -> LatencyMoversResult (copies), freeing the
    library's result."""
    (bf, bl), (cf, cl) = base, cur
    ppm = np.ascontiguousarray([int(round(float(q) * 1e6)) for q in quantiles], dtype=np.uint32)
    out = C.POINTER(_lib.sa_latency_movers_result)()
    obj._check(fn(obj._h, int(bf), int(bl), int(cf), int(cl), int(k), int(min_count), int(min_shift),
                  ppm.ctypes.data_as(_lib.u32p), len(ppm), _lib.SA_LATMOV_FALL if fall else 0, C.byref(out)), what)
    try:
        r = out.contents
        n, Q = int(r.n), int(r.n_q)
        col = lambda p, dt, *shape: (np.ctypeslib.as_array(p, shape=(n,) + shape).copy() if n
                                     else np.zeros((0,) + shape, dt))
        return LatencyMoversResult(
            (int(r.base_first), int(r.base_last)), (int(r.cur_first), int(r.cur_last)),
            bool(r.flags & _lib.SA_LATMOV_FALL), np.ctypeslib.as_array(r.q_ppm, shape=(Q,)).copy(),
            col(r.services, np.uint32), col(r.shift, np.int32), col(r.count_base, np.uint64),
            col(r.count_cur, np.uint64), col(r.q_bin_base, np.uint8, Q), col(r.q_bin_cur, np.uint8, Q),
            col(r.q_ns_base, np.uint64, Q), col(r.q_ns_cur, np.uint64, Q), int(r.n_services), int(r.n_eligible),
            int(r.n_matched), int(r.spans_base), int(r.spans_cur))
    finally:
        obj.lib.sa_latency_movers_result_free(out)


def _window_slo(obj, fn, what, first, last, widths, limit_ppm, thresholds_ns, services, min_count) -> SloResult:
    """sa_window_slo / sa_group_window_slo -> SloResult (copies), freeing the library's result."""
    sv = None if services is None else np.ascontiguousarray(services, dtype=np.uint32).reshape(-1)
    wd = np.ascontiguousarray(widths, dtype=np.uint32).reshape(-1)
    lim = np.ascontiguousarray(limit_ppm, dtype=np.uint32).reshape(-1)
    thr = np.ascontiguousarray(thresholds_ns, dtype=np.uint64).reshape(-1)
    if len(lim) != len(wd):
        raise ValueError(f"{what}: one limit_ppm a width")
    if len(thr) != (obj.config.n_services if sv is None else len(sv)):
        raise ValueError(f"{what}: one threshold a selected service")
    out = C.POINTER(_lib.sa_slo_result)()
    obj._check(fn(obj._h, int(first), int(last), wd.ctypes.data_as(_lib.u32p), lim.ctypes.data_as(_lib.u32p), len(wd),
                  None if sv is None else sv.ctypes.data_as(_lib.u32p), 0 if sv is None else len(sv),
                  thr.ctypes.data_as(_lib.u64p), int(min_count), 0, C.byref(out)), what)
    try:
        r = out.contents
        n, S, W = int(r.n_out), int(r.n_sel), int(r.n_widths)
        col = lambda p, *shape: np.ctypeslib.as_array(p, shape=shape).copy()
        return SloResult(
            int(r.first_window), int(r.last_window), int(r.min_count), col(r.services, S), col(r.widths, W),
            col(r.limit_ppm, W), col(r.threshold_ns, S), col(r.threshold_bin, S), col(r.effective_ns, S),
            col(r.total, n, W, S), col(r.slow, n, W, S), col(r.burning, n, S), col(r.alert_outputs, S))
    finally:
        obj.lib.sa_slo_result_free(out)


def _onset_result(obj, out) -> OnsetResult:
    """sa_onset_result -> OnsetResult (copies), freeing the library's result."""
    try:
        r = out.contents
        n = int(r.n)
        col = lambda p, dt: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, dt)
        return OnsetResult(
            int(r.first_window), int(r.last_window), bool(r.flags & _lib.SA_ONSET_FALL), int(r.q_ppm), int(r.min_count),
            col(r.services, np.uint32), col(r.onset_window, np.uint64), col(r.delta_ppm, np.int32),
            col(r.threshold_bin, np.uint8), col(r.effective_ns, np.uint64), col(r.total_before, np.uint64),
            col(r.slow_before, np.uint64), col(r.total_after, np.uint64), col(r.slow_after, np.uint64),
            int(r.n_services), int(r.n_eligible), int(r.n_matched), int(r.spans))
    finally:
        obj.lib.sa_onset_result_free(out)


def _window_latency_onset(obj, fn, what, first, last, k, quantile, thresholds_ns, min_count, min_delta_ppm,
                          fall) -> OnsetResult:
    """sa_window_latency_onset / sa_group_window_latency_onset -> OnsetResult."""
    thr = None if thresholds_ns is None else np.ascontiguousarray(thresholds_ns, dtype=np.uint64).reshape(-1)
    if thr is not None and len(thr) != obj.config.n_services:
        raise ValueError(f"{what}: one threshold a service")
    ppm = 0 if thr is not None else int(round(float(quantile) * 1e6))
    out = C.POINTER(_lib.sa_onset_result)()
    obj._check(fn(obj._h, int(first), int(last), int(k), ppm, None if thr is None else thr.ctypes.data_as(_lib.u64p),
                  int(min_count), int(min_delta_ppm), _lib.SA_ONSET_FALL if fall else 0, C.byref(out)), what)
    return _onset_result(obj, out)


_QUANTILES = (0.5, 0.95, 0.99)
_MOVER_QUANTILES = (0.99, 0.5, 0.95)  # the first one ranks


def _ptr(x) -> int:
    """Device pointer of a torch tensor, or an int passthrough."""
    if isinstance(x, int):
        return x
    return int(x.data_ptr())


def _expo_result(obj, rc, out, allow_drops, what) -> ExpoResult:
    """sa_exp_result -> ExpoResult (copies), freeing the library's result."""
    if rc not in (0, _lib.SA_EFULL) or not out:
        obj._check(rc if rc else _lib.SA_ESTATE, what)
    try:
        r = out.contents
        n, M = int(r.n_series), int(r.max_size)

        def arr(p, dt):
            return np.zeros(0, dtype=dt) if n == 0 else np.ctypeslib.as_array(p, shape=(n,)).copy()

        bk = np.zeros((0, M), np.uint64) if n == 0 else np.ctypeslib.as_array(r.bucket_counts, shape=(n, M))
        nb = arr(r.n_buckets, np.uint32)
        res = ExpoResult(arr(r.key_hash, np.uint64), arr(r.count, np.uint64), arr(r.zero_count, np.uint64),
                         arr(r.sum_ns, np.uint64), arr(r.sum, np.float64), arr(r.min, np.float64),
                         arr(r.max, np.float64), arr(r.scale, np.int32), arr(r.offset, np.int32),
                         [bk[i, : int(nb[i])].copy() for i in range(n)], rc)
    finally:
        obj.lib.sa_exp_result_free(out)
    if rc == _lib.SA_EFULL and not allow_drops:
        raise SpanAggError(rc, f"{what}: spans dropped (key table full); stats={obj.stats()}")
    return res


class Engine:
    def __init__(self, config: Optional[Config] = None, **kw):
        self.lib = _lib.load()
        self.config = config or Config(**kw)
        c, self._bounds_keepalive = self.config.to_c()
        h = C.c_void_p()
        rc = self.lib.sa_create(C.byref(c), C.byref(h))
        if rc != 0:
            raise SpanAggError(rc, "sa_create failed (is a gfx950 GPU visible?)")
        self._h = h
        self.n_buckets = len(self.config.bounds) + 1
        # dense-index engines (OPT_DENSE_IDS): the host dictionary that makes
        # the option transparent for host batches (ingest / ingest_async)
        self.dense = bool(self.config.options & _lib.OPT_DENSE_IDS)
        self.ids = DenseIds(self.stats()["table_capacity"]) if self.dense else None

    # -- lifecycle ---------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            self.lib.sa_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise SpanAggError(rc, f"{what}: {self.lib.sa_last_error(self._h).decode()}")

    # -- hot path ----------------------------------------------------------
    def bind_ids(self, index, key_hash):
        """sa_bind_ids (dense-index engines): index[j] stands for series
        key_hash[j] from now on, before every later ingest."""
        i = np.ascontiguousarray(index, dtype=np.uint64)
        h = np.ascontiguousarray(key_hash, dtype=np.uint64)
        if len(i) != len(h):
            raise ValueError("bind_ids: index and key_hash differ in length")
        self._check(self.lib.sa_bind_ids(self._h, i.ctypes.data_as(_lib.u64p), h.ctypes.data_as(_lib.u64p), len(i)),
                    "sa_bind_ids")

    def _host_columns(self, batch: SpanBatch):
        """The columns of a host batch as the engine takes them: on a dense
        engine the real hashes are encoded through self.ids and the new
        (index, hash) pairs bound first."""
        cols = batch.columns()
        if not self.dense:
            return cols
        ids, new_i, new_h = self.ids.encode(batch.key_hash)
        if len(new_i):
            self.bind_ids(new_i, new_h)
        return (np.ascontiguousarray(ids, dtype=np.uint64),) + tuple(cols[1:])

    def ingest(self, batch: SpanBatch):
        cols = self._host_columns(batch)
        b = _lib.sa_span_batch(*[c.ctypes.data for c in cols], len(batch))
        self._check(self.lib.sa_ingest(self._h, C.byref(b)), "sa_ingest")

    def ingest_async(self, batch: SpanBatch):
        """sa_ingest_async: columns in sa_host_alloc memory stay the engine's
        until the next ingest_async (or sync) returns."""
        cols = self._host_columns(batch)
        self._async_keepalive = cols  # (a dense engine's encoded ids, until the next call)
        b = _lib.sa_span_batch(*[c.ctypes.data for c in cols], len(batch))
        self._check(self.lib.sa_ingest_async(self._h, C.byref(b)), "sa_ingest_async")

    def ingest_device(self, key, start, end, w0, w1, meta, n: Optional[int] = None,
                      stream: Optional[int] = None):
        """Device-resident batch: torch tensors (or raw device pointers).  On
        a dense-index engine `key` holds indices as given: the caller encodes
        (self.ids or its own dictionary) and binds (bind_ids) first."""
        if n is None:
            n = int(key.numel())
        b = _lib.sa_span_batch(_ptr(key), _ptr(start), _ptr(end), _ptr(w0), _ptr(w1),
                               _ptr(meta), n)
        self._check(self.lib.sa_ingest_device(self._h, C.byref(b), C.c_void_p(stream or 0)),
                    "sa_ingest_device")

    def ingest_device_many(self, batches, stream: Optional[int] = None):
        """sa_ingest_device_many: device-resident batches in order, each a
        (key, start, end, w0, w1, meta[, n]) tuple of torch tensors or raw
        device pointers; one HIP graph of launches on small-table engines."""
        arr = (_lib.sa_span_batch * max(1, len(batches)))()
        for i, bt in enumerate(batches):
            cols = bt[:6]
            n = int(bt[6]) if len(bt) > 6 else int(cols[0].numel())
            arr[i] = _lib.sa_span_batch(*[_ptr(c) for c in cols], n)
        self._check(self.lib.sa_ingest_device_many(self._h, arr, len(batches), C.c_void_p(stream or 0)),
                    "sa_ingest_device_many")

    def join(self, stream: Optional[int] = None):
        """sa_join: order `stream` (a hipStream_t handle, None = the engine's)
        after every launch enqueued so far, the binned path's aggregates on
        the engine's own stream included (before timing events on `stream`)."""
        self._check(self.lib.sa_join(self._h, C.c_void_p(stream or 0)), "sa_join")

    def sync(self):
        self._check(self.lib.sa_sync(self._h), "sa_sync")

    # -- export ------------------------------------------------------------
    def flush(self, allow_drops: bool = False) -> RedResult:
        out = C.POINTER(_lib.sa_red_result)()
        rc = self.lib.sa_flush(self._h, C.byref(out))
        if self.dense:
            self.ids.flushed()
        return _red_result(self, rc, out, allow_drops, "sa_flush", self.lib.sa_flush)

    def window_read(self, window_id: int) -> SketchResult:
        out = C.POINTER(_lib.sa_sketch_result)()
        self._check(self.lib.sa_window_read(self._h, window_id, C.byref(out)), "sa_window_read")
        return _sketch_result(self.lib, out)

    def window_range(self, first: int, last: int, keys=None, registers: bool = False,
                     cells: bool = False) -> RangeResult:
        """sa_window_range: the resident windows first..last (inclusive)
        merged on the device -- per service the merged registers' histogram
        and estimate, and the summed count-min's estimate for each of `keys`
        (series hashes, also on a dense-index engine).  registers / cells:
        also the merged registers / the summed cells themselves."""
        return _window_range(self, self.lib.sa_window_range, "sa_window_range", first, last, keys, registers, cells)

    def window_series(self, first: int, last: int, width: int = 1, keys=None) -> SeriesResult:
        """sa_window_series: for every window t of first..last the answers of
        window_range(t - width + 1, t, keys), from one pass over the ring on
        the device (numpy copies; `keys` are series hashes, also on a
        dense-index engine)."""
        k = np.ascontiguousarray(() if keys is None else keys, dtype=np.uint64).reshape(-1)
        out = C.POINTER(_lib.sa_series_result)()
        self._check(self.lib.sa_window_series(self._h, int(first), int(last), int(width),
                                              k.ctypes.data_as(_lib.u64p) if len(k) else None, len(k), 0,
                                              C.byref(out)), "sa_window_series")
        try:
            r = out.contents
            n, S, p = int(r.n_out), int(r.n_services), int(r.hll_p)
            return SeriesResult(
                int(r.first_window), int(r.last_window), int(r.width),
                np.ctypeslib.as_array(r.hll_hist, shape=(n, S, _lib.SA_HLL_HIST_BINS)).copy(),
                np.ctypeslib.as_array(r.distinct, shape=(n, S)).copy(),
                np.ctypeslib.as_array(r.error_spans, shape=(n,)).copy(),
                np.ctypeslib.as_array(r.errors, shape=(n, len(k))).copy() if len(k) else np.zeros((n, 0), np.uint64),
                k, p)
        finally:
            self.lib.sa_series_result_free(out)

    def window_top(self, first: int, last: int, k: int = 10, min_count: int = 1) -> TopResult:
        """sa_window_top: the k series with the largest estimate of the
        count-min summed over windows first..last, among the series resident
        in the key table (those seen since the last reclaim) with an estimate
        >= min_count -- scanned, selected and sorted on the device."""
        return _window_top(self, self.lib.sa_window_top, "sa_window_top", first, last, k, min_count)

    def window_movers(self, base, cur, k: int = 10, min_score: int = 1, fall: bool = False) -> MoversResult:
        """sa_window_movers: the k series whose ERROR spans per window rose
        most (fall: fell most) from the windows base = (first, last) to the
        windows cur = (first, last), among the series resident in the key
        table with a score >= min_score -- one scan of the table against both
        ranges' summed count-mins, selected and sorted on the device."""
        return _window_movers(self, self.lib.sa_window_movers, "sa_window_movers", base, cur, k, min_score, fall)

    def window_error_onset(self, first: int, last: int, k: int = 10, min_count: int = 1, min_score: int = 1,
                           fall: bool = False) -> ErrorOnsetResult:
        """sa_window_error_onset: for every series resident in the key table
        with at least min_count estimated ERROR spans over windows first..last,
        the split of the range with the largest window_movers score (the
        latest among equal ones), and the k series whose best score is largest
        (>= min_score) with the window at which "after" begins -- one walk
        over the ring's count-mins per series, selected and sorted on the
        device."""
        return _window_error_onset(self, self.lib.sa_window_error_onset, "sa_window_error_onset", first, last, k,
                                   min_count, min_score, fall)

    def window_overlap(self, first: int, last: int, services=None) -> OverlapResult:
        """sa_window_overlap: the traces every pair of `services` (ids, at most
        OVERLAP_MAX_SERVICES; None: every service of an engine with no more
        than that) shares over windows first..last -- registers max-merged
        per service, then the pairwise maxima and their histograms, on the
        device."""
        return _window_overlap(self, self.lib.sa_window_overlap, "sa_window_overlap", first, last, services)

    def window_latency(self, first: int, last: int, services=None, quantiles=_QUANTILES,
                       hist: bool = False) -> LatencyResult:
        """sa_window_latency as a range query (OPT_WINDOW_LATENCY engines): one
        output over the windows first..last -- per service of `services` (ids;
        None: every service) the spans counted there and each quantile's
        histogram bin and upper bound in ns.  hist: also the summed bins."""
        return _window_latency(self, self.lib.sa_window_latency, "sa_window_latency", last, last, last - first + 1,
                               services, quantiles, hist)

    def window_latency_series(self, first: int, last: int, width: int = 1, services=None, quantiles=_QUANTILES,
                              hist: bool = False) -> LatencyResult:
        """sa_window_latency: for every window t of first..last the answers of
        window_latency(t - width + 1, t), from sliding sums on the device."""
        return _window_latency(self, self.lib.sa_window_latency, "sa_window_latency", first, last, width, services,
                               quantiles, hist)

    def window_latency_movers(self, base, cur, k: int = 10, quantiles=_MOVER_QUANTILES, min_count: int = 1,
                              min_shift: int = 1, fall: bool = False) -> LatencyMoversResult:
        """sa_window_latency_movers (OPT_WINDOW_LATENCY engines): the k
        services whose quantiles[0] rose most histogram bins (fall: fell most)
        from the windows base = (first, last) to the windows cur = (first,
        last), among the services with at least min_count spans in both and a
        shift >= min_shift -- both ranges summed, scored, selected and sorted
        on the device; every quantile's bin and bound of the returned rows."""
        return _window_latency_movers(self, self.lib.sa_window_latency_movers, "sa_window_latency_movers", base, cur, k,
                                      quantiles, min_count, min_shift, fall)

    def window_slo(self, first: int, last: int, widths, limit_ppm, thresholds_ns, services=None,
                   min_count: int = 1) -> SloResult:
        """sa_window_slo (OPT_WINDOW_LATENCY engines): for every window t of
        first..last, every width of `widths` (at most SLO_MAX_WIDTHS) and every
        service of `services` (ids; None: every service) the spans of windows
        t - width + 1 .. t and those slower than the service's entry of
        thresholds_ns, and whether width w burns: slow * 10^6 > limit_ppm[w] *
        total with at least min_count spans.  The ring is read once whatever
        the widths; only the sums and the verdicts cross the bus."""
        return _window_slo(self, self.lib.sa_window_slo, "sa_window_slo", first, last, widths, limit_ppm, thresholds_ns,
                           services, min_count)

    def window_latency_onset(self, first: int, last: int, k: int = 10, quantile: float = 0.95, thresholds_ns=None,
                             min_count: int = 1, min_delta_ppm: int = 1, fall: bool = False) -> OnsetResult:
        """sa_window_latency_onset (OPT_WINDOW_LATENCY engines): for every
        service the window inside first..last at which its share of slow spans
        changed -- the split with the largest S_after * N_before - S_before *
        N_after among those with at least min_count spans on both sides, the
        latest on ties -- and the k services whose share rose most (fall: fell),
        by at least min_delta_ppm.  Slow: above the bin of the service's entry
        of thresholds_ns (one a service), or with thresholds_ns None above the
        bin of `quantile` of the service's spans over the whole range."""
        return _window_latency_onset(self, self.lib.sa_window_latency_onset, "sa_window_latency_onset", first, last, k,
                                     quantile, thresholds_ns, min_count, min_delta_ppm, fall)

    def onset_probe(self, pairs, k: int = 10, min_count: int = 1, min_delta_ppm: int = 1, fall: bool = False) -> OnsetResult:
        """Diagnostic (sa_onset_probe): window_latency_onset's scan and select
        on `pairs` [n_sel][n_cov][2] u64 -- (total, slow) a service and window
        -- instead of a ring's; windows count from 0, threshold_bin and
        effective_ns come back 0."""
        a = np.ascontiguousarray(pairs, dtype=np.uint64)
        if a.ndim != 3 or a.shape[2] != 2:
            raise ValueError("sa_onset_probe: pairs [n_sel][n_cov][2]")
        out = C.POINTER(_lib.sa_onset_result)()
        self._check(self.lib.sa_onset_probe(self._h, a.ctypes.data_as(_lib.u64p), a.shape[0], a.shape[1], int(k),
                                            int(min_count), int(min_delta_ppm), _lib.SA_ONSET_FALL if fall else 0,
                                            C.byref(out)), "sa_onset_probe")
        return _onset_result(self, out)

    def flush_exp(self, allow_drops: bool = False) -> ExpoResult:
        out = C.POINTER(_lib.sa_exp_result)()
        rc = self.lib.sa_flush_exp(self._h, C.byref(out))
        return _expo_result(self, rc, out, allow_drops, "sa_flush_exp")

    def reclaim_keys(self, force: bool = False):
        """sa_reclaim_keys: empty the key table (force) or do the flush-time
        policy (more than half full); only right after a flush."""
        self._check(self.lib.sa_reclaim_keys(self._h, int(force)), "sa_reclaim_keys")

    def key_union_probe(self, ids) -> np.ndarray:
        """Diagnostic: the group flush's device key union (sa_key_union_probe)
        of `ids` -- their distinct non-zero values, ascending."""
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.empty(max(1, len(a)), dtype=np.uint64)
        n = C.c_uint64(0)
        self._check(self.lib.sa_key_union_probe(self._h, a.ctypes.data_as(_lib.u64p), len(a),
                                                out.ctypes.data_as(_lib.u64p), C.byref(n)), "sa_key_union_probe")
        return out[: n.value].copy()

    def expo_probe(self, values, scales):
        """GPU bucket index and Go math.Log of each value (diagnostic)."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        s = np.ascontiguousarray(scales, dtype=np.int32)
        idx = np.zeros(len(v), dtype=np.int32)
        logs = np.zeros(len(v), dtype=np.float64)
        self._check(self.lib.sa_expo_probe(self._h, v.ctypes.data_as(_lib.f64p), s.ctypes.data_as(C.POINTER(C.c_int32)),
                                           len(v), idx.ctypes.data_as(C.POINTER(C.c_int32)),
                                           logs.ctypes.data_as(_lib.f64p)), "sa_expo_probe")
        return idx, logs

    def expo_fast_probe(self, d_ns, scales, log2_err=True):
        """The counting kernel's bucket-index fast path (diagnostic): (fast,
        exact, max log2 error) -- fast[i] is INT32_MIN where it defers to the
        exact path; the error is the hardware log2's over every float in [1, 2)."""
        d = np.ascontiguousarray(d_ns, dtype=np.uint64)
        s = np.ascontiguousarray(scales, dtype=np.int32)
        fast = np.zeros(len(d), dtype=np.int32)
        exact = np.zeros(len(d), dtype=np.int32)
        err = C.c_double(0.0)
        self._check(self.lib.sa_expo_fast_probe(self._h, d.ctypes.data_as(_lib.u64p),
                                                s.ctypes.data_as(C.POINTER(C.c_int32)), len(d),
                                                fast.ctypes.data_as(C.POINTER(C.c_int32)),
                                                exact.ctypes.data_as(C.POINTER(C.c_int32)),
                                                C.byref(err) if log2_err else None), "sa_expo_fast_probe")
        return fast, exact, err.value

    def window_advance(self, new_base: int):
        self._check(self.lib.sa_window_advance(self._h, int(new_base)), "sa_window_advance")

    def stats(self) -> dict:
        s = _lib.sa_stats()
        self._check(self.lib.sa_get_stats(self._h, C.byref(s)), "sa_get_stats")
        return {name: int(getattr(s, name)) for name, _ in _lib.sa_stats._fields_ if name != "pad"}

    def debug_geometry(self) -> dict:
        """sa_debug_geometry: which ingest kernel this engine runs -- path and
        kernel by name (_lib.PATH_NAMES, _lib.KERNEL_NAMES), block, grid_max,
        log2cap, lb_shift, lb_n (0: no HLL filter), error_table, lds_bytes; and
        the exponential histograms' counting pass -- expo_count (_lib.EXPO_COUNT_*:
        0 none, 1 slab counting, 2 cached-probe, 3 the HBM passes), expo_entries,
        expo_bin_slots, expo_bins."""
        g = _lib.sa_debug_geometry_info()
        self._check(self.lib.sa_debug_geometry(self._h, C.byref(g)), "sa_debug_geometry")
        d = {name: int(getattr(g, name)) for name, _ in g._fields_}
        d["path"], d["kernel"] = _lib.PATH_NAMES[g.path], _lib.KERNEL_NAMES[g.kernel]
        d["error_table"] = bool(g.error_table)
        return d

    # -- multi-GPU merge hooks (device pointers) ----------------------------
    def export_keys(self, d_keys, cap: int, stream: Optional[int] = None) -> int:
        n = C.c_uint64(0)
        self._check(self.lib.sa_export_keys(self._h, C.c_void_p(_ptr(d_keys) if cap else 0), cap,
                                            C.byref(n), C.c_void_p(stream or 0)), "sa_export_keys")
        return int(n.value)

    def gather_dense(self, d_keys, n: int, d_rows, reset: bool, stream: Optional[int] = None):
        self._check(self.lib.sa_gather_dense(self._h, C.c_void_p(_ptr(d_keys) if n else 0), n,
                                             C.c_void_p(_ptr(d_rows) if n else 0), int(reset),
                                             C.c_void_p(stream or 0)), "sa_gather_dense")

    def window_export(self, window_id: int, d_hll, d_cms, stream: Optional[int] = None):
        self._check(self.lib.sa_window_export(self._h, window_id, C.c_void_p(_ptr(d_hll)),
                                              C.c_void_p(_ptr(d_cms)), C.c_void_p(stream or 0)),
                    "sa_window_export")


class Group:
    """One engine per GPU behind one handle (include/spanagg.h sa_group_*):
    host batches shard by trace id (trace_w1 % n), flush and window reads
    return the merge (RCCL over distinct devices, device copies otherwise)."""

    def __init__(self, devices: Sequence[int], config: Optional[Config] = None, **kw):
        self.lib = _lib.load()
        self.config = config or Config(**kw)
        c, self._bounds_keepalive = self.config.to_c()
        devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self.lib.sa_group_create(C.byref(c), devs, len(devices), C.byref(h))
        if rc != 0:
            raise SpanAggError(rc, "sa_group_create failed (are the gfx950 GPUs visible?)")
        self._h = h
        self.n_buckets = len(self.config.bounds) + 1

    def close(self):
        if getattr(self, "_h", None):
            self.lib.sa_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise SpanAggError(rc, f"{what}: {self.lib.sa_group_last_error(self._h).decode()}")

    @property
    def size(self) -> int:
        return int(self.lib.sa_group_size(self._h))

    @property
    def uses_rccl(self) -> bool:
        return bool(self.lib.sa_group_uses_rccl(self._h))

    def ingest(self, batch: SpanBatch):
        b = _lib.sa_span_batch(*[c.ctypes.data for c in batch.columns()], len(batch))
        self._check(self.lib.sa_group_ingest(self._h, C.byref(b)), "sa_group_ingest")

    def ingest_device(self, key, start, end, w0, w1, meta, n: Optional[int] = None, src: int = 0,
                      stream: Optional[int] = None):
        """sa_group_ingest_device: a batch in HBM of member `src`'s device
        (torch tensors or raw device pointers), partitioned by trace id on
        that device and ingested by every member on its own stream."""
        if n is None:
            n = int(key.numel())
        b = _lib.sa_span_batch(_ptr(key), _ptr(start), _ptr(end), _ptr(w0), _ptr(w1), _ptr(meta), n)
        self._check(self.lib.sa_group_ingest_device(self._h, C.byref(b), int(src), C.c_void_p(stream or 0)),
                    "sa_group_ingest_device")

    def sync(self):
        self._check(self.lib.sa_group_sync(self._h), "sa_group_sync")

    def flush(self, allow_drops: bool = False) -> RedResult:
        out = C.POINTER(_lib.sa_red_result)()
        rc = self.lib.sa_group_flush(self._h, C.byref(out))
        return _red_result(self, rc, out, allow_drops, "sa_group_flush")

    def flush_exp(self, allow_drops: bool = False) -> ExpoResult:
        """sa_group_flush_exp: the members' exponential histograms, folded."""
        out = C.POINTER(_lib.sa_exp_result)()
        rc = self.lib.sa_group_flush_exp(self._h, C.byref(out))
        return _expo_result(self, rc, out, allow_drops, "sa_group_flush_exp")

    def window_read(self, window_id: int) -> SketchResult:
        out = C.POINTER(_lib.sa_sketch_result)()
        self._check(self.lib.sa_group_window_read(self._h, window_id, C.byref(out)), "sa_group_window_read")
        return _sketch_result(self.lib, out)

    def window_range(self, first: int, last: int, keys=None, registers: bool = False,
                     cells: bool = False) -> RangeResult:
        """sa_group_window_range: Engine.window_range over the members' merge."""
        return _window_range(self, self.lib.sa_group_window_range, "sa_group_window_range", first, last, keys,
                             registers, cells)

    def window_top(self, first: int, last: int, k: int = 10, min_count: int = 1) -> TopResult:
        """sa_group_window_top: Engine.window_top over the members' merge
        (n_resident and n_matched summed over the members)."""
        return _window_top(self, self.lib.sa_group_window_top, "sa_group_window_top", first, last, k, min_count)

    def window_movers(self, base, cur, k: int = 10, min_score: int = 1, fall: bool = False) -> MoversResult:
        """sa_group_window_movers: Engine.window_movers over the members' merge
        (n_resident and n_matched are summed over members)."""
        return _window_movers(self, self.lib.sa_group_window_movers, "sa_group_window_movers", base, cur, k, min_score,
                              fall)

    def window_error_onset(self, first: int, last: int, k: int = 10, min_count: int = 1, min_score: int = 1,
                           fall: bool = False) -> ErrorOnsetResult:
        """sa_group_window_error_onset: Engine.window_error_onset over the
        members' merge -- every window's cells summed across members, a scan
        on every member, the rows merged on the host."""
        return _window_error_onset(self, self.lib.sa_group_window_error_onset, "sa_group_window_error_onset", first,
                                   last, k, min_count, min_score, fall)

    def window_overlap(self, first: int, last: int, services=None) -> OverlapResult:
        """sa_group_window_overlap: Engine.window_overlap over the members' merge."""
        return _window_overlap(self, self.lib.sa_group_window_overlap, "sa_group_window_overlap", first, last,
                               services)

    def window_latency(self, first: int, last: int, services=None, quantiles=_QUANTILES,
                       hist: bool = False) -> LatencyResult:
        """sa_group_window_latency as a range query: Engine.window_latency
        over the members' summed histograms."""
        return _window_latency(self, self.lib.sa_group_window_latency, "sa_group_window_latency", last, last,
                               last - first + 1, services, quantiles, hist)

    def window_latency_series(self, first: int, last: int, width: int = 1, services=None, quantiles=_QUANTILES,
                              hist: bool = False) -> LatencyResult:
        """sa_group_window_latency: Engine.window_latency_series over the
        members' summed histograms."""
        return _window_latency(self, self.lib.sa_group_window_latency, "sa_group_window_latency", first, last, width,
                               services, quantiles, hist)

    def window_latency_movers(self, base, cur, k: int = 10, quantiles=_MOVER_QUANTILES, min_count: int = 1,
                              min_shift: int = 1, fall: bool = False) -> LatencyMoversResult:
        """sa_group_window_latency_movers: Engine.window_latency_movers over
        the members' summed histograms."""
        return _window_latency_movers(self, self.lib.sa_group_window_latency_movers, "sa_group_window_latency_movers",
                                      base, cur, k, quantiles, min_count, min_shift, fall)

    def window_slo(self, first: int, last: int, widths, limit_ppm, thresholds_ns, services=None,
                   min_count: int = 1) -> SloResult:
        """sa_group_window_slo: Engine.window_slo over the members' summed
        (total, slow) pairs."""
        return _window_slo(self, self.lib.sa_group_window_slo, "sa_group_window_slo", first, last, widths, limit_ppm,
                           thresholds_ns, services, min_count)

    def window_latency_onset(self, first: int, last: int, k: int = 10, quantile: float = 0.95, thresholds_ns=None,
                             min_count: int = 1, min_delta_ppm: int = 1, fall: bool = False) -> OnsetResult:
        """sa_group_window_latency_onset: Engine.window_latency_onset over the
        members' summed histograms (the pooled threshold) and summed pairs."""
        return _window_latency_onset(self, self.lib.sa_group_window_latency_onset, "sa_group_window_latency_onset", first,
                                     last, k, quantile, thresholds_ns, min_count, min_delta_ppm, fall)

    def window_advance(self, new_base: int):
        self._check(self.lib.sa_group_window_advance(self._h, int(new_base)), "sa_group_window_advance")

    def stats(self) -> dict:
        s = _lib.sa_stats()
        self._check(self.lib.sa_group_get_stats(self._h, C.byref(s)), "sa_group_get_stats")
        return {name: int(getattr(s, name)) for name, _ in _lib.sa_stats._fields_ if name != "pad"}
