"""Latency movers over the window ring (sa_window_latency_movers): the cases'
workloads and a numpy restatement of the call over latency_util.window_hists,
shared by tests/test_window_latency_movers_host.py (what the inputs can catch,
against the plain-Python sketch.latency_movers) and
tests/test_gpu_window_latency_movers.py (the kernels).

  spans      a batch from (window, service, duration) columns: key 0 and
             status OK, so it reaches the latency ring and nothing else
  drawn      log-uniform durations whose scale drifts per (service, window),
             so a range's quantile differs from another's
  rank       the call over two summed [n][256] arrays of the services `ids`
             (every other service has no span and is not eligible)
  expected   rank over the windows of a latency_util.window_hists reference

The `wrong` switches of rank / expected build references with a known mistake:

  ignore_count         ordered by (shift, service): count_cur not a key
  rank_q1              ranked by q_ppm[1] instead of q_ppm[0]
  min_count_one_range  min_count applied to the current range only
  mean_of_windows      the mean (rounded down) of the windows' own quantile bins
                       instead of the quantile of the summed range
  fall_not_flipped     the sign of the shift kept under fall
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import latency_util as lu
from geometry_util import ring_start
from spanagg import Config, SpanBatch, pack_meta, sketch
from spanagg._lib import OPT_WINDOW_LATENCY

U = np.uint64
COUNT_CLAMP = (1 << 48) - 1
WRONG = ("ignore_count", "rank_q1", "min_count_one_range", "mean_of_windows", "fall_not_flipped")
PPM3 = (990_000, 500_000, 950_000)
Q3 = tuple(p / 1e6 for p in PPM3)
LONG_LENGTHS = (1, 2, 3, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 255, 256)  # 8 windows a stripe, doubling
SERVICE_COUNTS = (1, 3, 5, 64, 257, 1000)


def lo_of(b) -> int:
    return sketch.latency_bin_bounds(int(b))[0]


def spans(cfg, window, service, duration, keys=64) -> SpanBatch:
    """One span per element: it ends 5 ns into `window` and lasts `duration`;
    status OK, the series ids 1..keys in turn (keys=0: key 0, a span that
    reaches the latency ring and neither the key table nor the RED counters)."""
    window, service, duration = (np.asarray(x) for x in (window, service, duration))
    n = len(window)
    end = window.astype(np.uint64) * U(cfg.window_ns) + U(5)
    ids = np.arange(1, n + 1, dtype=np.uint64)
    key = U(1) + ids % U(keys) if keys else np.zeros(n, np.uint64)
    return SpanBatch(key, end - duration.astype(np.uint64), end, ids, ids, pack_meta(service, [0] * n, [0] * n))


def drawn(seed, cfg, base, n) -> SpanBatch:
    """n spans over the ring from `base`: services and windows uniform,
    durations log-uniform over 1 us .. 1 s times a factor 2^-3 .. 2^3 drawn
    per (service, window)."""
    rng = np.random.default_rng(seed)
    S, W = cfg.n_services, cfg.n_windows
    svc, win = rng.integers(0, S, n), rng.integers(0, W, n)
    factor = np.exp2(rng.uniform(-3, 3, (S, W)))
    dur = np.exp(rng.uniform(np.log(1e3), np.log(1e9), n)) * factor[svc, win]
    return spans(cfg, base + win, svc, dur.astype(np.uint64))


def lat_cfg(S, W, hll_p=4, **kw) -> Config:
    return Config(n_services=S, n_windows=W, hll_p=hll_p, key_capacity=1000, options=OPT_WINDOW_LATENCY, **kw)


def rank(hb, hc, ids, n_services, k, ppm, min_count=1, min_shift=1, fall=False, wrong=None, per_window=None):
    """hb, hc [n][256]: the summed rows of services ids [n] (ascending).
    per_window: ([nb][n][256], [nc][n][256]) for wrong="mean_of_windows"."""
    ids = np.asarray(ids, dtype=np.uint32)
    cb, qb, nsb = lu.quantile_bins(hb, ppm)
    cc, qc, nsc = lu.quantile_bins(hc, ppm)
    if wrong == "mean_of_windows":
        qb, qc = ((lu.quantile_bins(h, ppm)[1].astype(np.int64).sum(axis=0) // len(h)).astype(np.uint8) for h in per_window)
        nsb, nsc = lu.BIN_HI[qb], lu.BIN_HI[qc]
    col = 1 if wrong == "rank_q1" and len(ppm) > 1 else 0
    shift = qc[:, col].astype(np.int64) - qb[:, col].astype(np.int64)
    if fall and wrong != "fall_not_flipped":
        shift = -shift
    mc, ms = max(int(min_count), 1), max(int(min_shift), 1)
    elig = (cc >= U(mc)) if wrong == "min_count_one_range" else (cb >= U(mc)) & (cc >= U(mc))
    match = np.flatnonzero(elig & (shift >= ms))
    clamped = np.minimum(cc[match], U(COUNT_CLAMP)).astype(np.int64)
    keys = (ids[match], -shift[match]) if wrong == "ignore_count" else (ids[match], -clamped, -shift[match])
    order = match[np.lexsort(keys)]
    top = order[:k]
    return SimpleNamespace(services=ids[top], shift=shift[top].astype(np.int32), count_base=cb[top], count_cur=cc[top],
                           q_bin_base=qb[top], q_bin_cur=qc[top], q_ns_base=nsb[top], q_ns_cur=nsc[top],
                           n_services=int(n_services), n_eligible=int(elig.sum()), n_matched=len(order),
                           spans_base=int(cb.sum(dtype=np.uint64)), spans_cur=int(cc.sum(dtype=np.uint64)),
                           order=ids[order], order_shift=shift[order], order_count=cc[order])


def expected(ref, cfg, base, cur, k, ppm, min_count=1, min_shift=1, fall=False, wrong=None):
    """What window_latency_movers(base, cur, k, ppm / 1e6, min_count, min_shift,
    fall) must return over the reference `ref` (latency_util.window_hists)."""
    wb, wc = lu.ring_hists(ref, cfg, *base), lu.ring_hists(ref, cfg, *cur)
    return rank(wb.sum(axis=0, dtype=np.uint64), wc.sum(axis=0, dtype=np.uint64), np.arange(cfg.n_services),
                cfg.n_services, k, ppm, min_count, min_shift, fall, wrong, (wb, wc))


def items(m):
    return [(int(s), int(d), int(b), int(c), tuple(int(x) for x in qb), tuple(int(x) for x in qc))
            for s, d, b, c, qb, qc in zip(m.services, m.shift, m.count_base, m.count_cur, m.q_bin_base, m.q_bin_cur)]


FIELDS = ("services", "shift", "count_base", "count_cur", "q_bin_base", "q_bin_cur", "q_ns_base", "q_ns_cur")
COUNTERS = ("n_services", "n_eligible", "n_matched", "spans_base", "spans_cur")


def assert_latency_movers(res, want, what=""):
    """A LatencyMoversResult against rank()'s reference: every column and counter, bit for bit."""
    assert res.services.dtype == np.uint32 and res.shift.dtype == np.int32 and res.q_bin_base.dtype == np.uint8, what
    for f in FIELDS:
        got, ref = getattr(res, f), getattr(want, f)
        assert got.shape == ref.shape and np.array_equal(got, ref), (f, what)
    for f in COUNTERS:
        assert getattr(res, f) == getattr(want, f), (f, what, getattr(res, f), getattr(want, f))
    assert (res.shift >= 1).all(), what


def same(a, b):
    for f in FIELDS + ("q_ppm",):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    for f in COUNTERS + ("base", "cur", "fall"):
        assert getattr(a, f) == getattr(b, f), f


# ---- the cases: cfg, steps [(ring base, batch)], base (the final ring's first
# window), calls [(base range, cur range, k, ppm, min_count, min_shift, fall)] ----
# crafted: service -> (bin of its slowest span in the baseline range, in the current one, spans in the current one)
CRAFTED = {0: (40, 100, 3), 1: (50, 80, 5), 2: (90, 60, 4), 3: (None, 70, 6), 4: (20, 21, 3), 5: (10, 5, 2)}
CRAFTED_RISE, CRAFTED_FALL = [(0, 60), (1, 30), (4, 1)], [(2, 30), (5, 5)]


def _crafted():
    """W = 8, S = 6; the baseline is the first four windows, the current range
    the last four.  A service has 4 spans in the baseline (n in the current
    range): two at the lower bound of its bin, in two windows, the others two
    bins below in the other windows -- the 0.99 quantile of a range is the
    slowest span's bin, of a single window not always."""
    cfg = lat_cfg(6, 8)
    w0 = ring_start(cfg)
    win, svc, dur = [], [], []
    for s, (bb, bc, n) in CRAFTED.items():
        for first, b, m in ((w0, bb, 4), (w0 + 4, bc, n)):
            for i in range(m if b is not None else 0):
                win.append(first + i % 4), svc.append(s), dur.append(lo_of(b if i < 2 else b - 2))
    B, C = (w0, w0 + 3), (w0 + 4, w0 + 7)
    calls = [(B, C, 10, PPM3, 1, 1, False), (B, C, 10, PPM3, 1, 1, True), (B, C, 2, PPM3, 1, 1, False),
             (B, C, 10, PPM3, 1, 30, False), (B, C, 10, PPM3, 1, 31, False), (B, C, 10, PPM3, 1, 256, False),
             (B, C, 10, PPM3, 3, 1, False), (B, C, 10, PPM3, 4, 1, False), (B, C, 10, PPM3, 5, 1, False),
             (B, C, 10, PPM3, 4, 1, True), (B, C, 10, PPM3, 5, 1, True), (B, C, 10, (500_000,), 1, 1, False)]
    return cfg, [(w0, spans(cfg, win, svc, dur))], w0, calls


# ties: service -> (shift, spans in the current range); every baseline is 2 spans at bin 30
TIES = {0: (10, 7), 1: (10, 8), 2: (10, 7), 3: (10, 9), 4: (10, 5), 5: (10, 5), 6: (10, 5), 7: (10, 5),
        8: (12, 5), 9: (12, 5), 10: (12, 5), 11: (12, 5)}
TIES_ORDER = [8, 9, 10, 11, 3, 1, 0, 2, 4, 5, 6, 7]
TIES_KS = (2, 5, 7, 10)  # inside (12, 5) by id; inside shift 10 by count; inside (10, 7) by id; inside (10, 5) by id


def _ties():
    cfg = lat_cfg(12, 4)
    w0 = ring_start(cfg)
    win, svc, dur = [], [], []
    for s, (shift, n) in TIES.items():
        for i in range(2):
            win.append(w0 + i), svc.append(s), dur.append(lo_of(30))
        for i in range(n):
            win.append(w0 + 2 + i % 2), svc.append(s), dur.append(lo_of(30 + shift))
    B, C = (w0, w0 + 1), (w0 + 2, w0 + 3)
    return cfg, [(w0, spans(cfg, win, svc, dur))], w0, [(B, C, k, PPM3, 1, 1, False) for k in TIES_KS]


def _services(S):
    cfg = lat_cfg(S, 8)
    w0 = ring_start(cfg)
    B, C = (w0, w0 + 3), (w0 + 4, w0 + 7)
    return cfg, [(w0, drawn(zlib.crc32(b"latmov_services") + S, cfg, w0, 20_000 + 40 * S))], w0, \
        [(B, C, 64, PPM3, 1, 1, False), (B, C, 64, PPM3, 20, 2, True)]


def _ranges():
    """W = 16, the ring moved by 11: the resident windows wrap the slots."""
    cfg = lat_cfg(10, 16)
    w0 = ring_start(cfg)
    b = w0 + 11
    steps = [(w0, drawn(zlib.crc32(b"latmov_ranges"), cfg, w0, 30_000)),
             (b, drawn(zlib.crc32(b"latmov_ranges2"), cfg, b, 30_000))]
    pairs = [((b, b + 9), (b + 5, b + 15)),    # overlapping
             ((b + 2, b + 9), (b + 2, b + 9)),   # equal
             ((b, b + 1), (b + 3, b + 13)),      # of unequal length
             ((b + 10, b + 15), (b, b + 4)),     # base after cur
             ((b + 4, b + 4), (b + 5, b + 5)),   # of length 1 (the slots' wrap lies between them)
             ((b, b + 15), (b + 15, b + 15)),    # of length W, and the last window
             ((b + 7, b + 7), (b, b + 15))]
    return cfg, steps, b, [(B, C, 10, PPM3, 1, 1, fall) for B, C in pairs for fall in (False, True)]


def _long():
    """W = 256, S = 3: the baseline the first `n` windows, the current range the last n."""
    cfg = lat_cfg(3, 256)
    w0 = ring_start(cfg)
    calls = [((w0, w0 + n - 1), (w0 + 256 - n, w0 + 255), 3, PPM3, 1, 1, fall) for n in LONG_LENGTHS
             for fall in (False, True)]
    return cfg, [(w0, drawn(zlib.crc32(b"latmov_long"), cfg, w0, 60_000))], w0, calls


SELECT_S, SELECT_K = 5000, 4096


def _select():
    """S = 5,000, W = 4: every service but each 50th rises by 1, 2 or 3 bins
    with 1..4 spans in the current range -- twelve classes of equal (shift,
    count_cur), some four hundred services each; each 50th falls."""
    cfg = lat_cfg(SELECT_S, 4)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"latmov_select"))
    s = np.arange(SELECT_S)
    shift = np.where(s % 50 == 49, -2, rng.integers(1, 4, SELECT_S))
    n_cur = rng.integers(1, 5, SELECT_S)
    base_bin = rng.integers(20, 200, SELECT_S)
    win = np.concatenate([w0 + s % 2, np.repeat(w0 + 2, n_cur.sum()) + np.concatenate([np.arange(n) % 2 for n in n_cur])])
    svc = np.concatenate([s, np.repeat(s, n_cur)])
    bins = np.concatenate([base_bin, np.repeat(base_bin + shift, n_cur)])
    dur = np.array([lo_of(b) for b in range(256)], dtype=np.uint64)[bins]
    B, C = (w0, w0 + 1), (w0 + 2, w0 + 3)
    return cfg, [(w0, spans(cfg, win, svc, dur))], w0, [(B, C, k, PPM3, 1, 1, False) for k in (SELECT_K, 1, 10)]


BUILDERS = dict(crafted=_crafted, ties=_ties, ranges=_ranges, long=_long, select=_select,
                **{f"services{S}": functools.partial(_services, S) for S in SERVICE_COUNTS})
HOST_CASES = tuple(BUILDERS)


@functools.lru_cache(maxsize=3)
def case(name):
    cfg, steps, base, calls = BUILDERS[name]()
    return SimpleNamespace(name=name, cfg=cfg, steps=steps, base=base, calls=calls, ref=lu.window_hists(cfg, steps))


def want(c, call, wrong=None):
    B, C, k, ppm, mc, ms, fall = call
    return expected(c.ref, c.cfg, B, C, k, ppm, mc, ms, fall, wrong)


def run(x, call):
    """The call on an engine or a group."""
    B, C, k, ppm, mc, ms, fall = call
    return x.window_latency_movers(B, C, k, [p / 1e6 for p in ppm], mc, ms, fall)


def loaded(c, cls=None, *a, cfg=None):
    """A fresh engine (or cls(*a, cfg)) after the case's steps, host ingest."""
    from spanagg import Engine
    x = (cls or Engine)(*a, cfg or c.cfg)
    try:
        for base, batch in c.steps:
            x.window_advance(base)
            x.ingest(batch)
    except BaseException:
        x.close()
        raise
    return x


# at the bound: S = 65,536, W = 4 (the 512 MiB ring); the reference holds the used services only
BOUND_S, BOUND_USED = 65_536, 300


@functools.lru_cache(maxsize=1)
def bound_case():
    cfg = lat_cfg(BOUND_S, 4)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"latmov_bound"))
    ids = np.unique(np.concatenate([rng.integers(0, BOUND_S, BOUND_USED), [0, BOUND_S - 1]]))
    small = dataclasses.replace(cfg, n_services=len(ids))
    compact = drawn(zlib.crc32(b"latmov_bound_spans"), small, w0, 12 * len(ids))
    svc = ids[(compact.meta & np.uint32(0xFFFF)).astype(np.int64)]
    batch = SpanBatch(compact.key_hash, compact.start_ns, compact.end_ns, compact.trace_w0, compact.trace_w1,
                      pack_meta(svc, [0] * len(svc), [0] * len(svc)))
    ref = lu.window_hists(small, [(w0, compact)])
    B, C = (w0, w0 + 1), (w0 + 2, w0 + 3)
    hb = lu.ring_hists(ref, small, *B).sum(axis=0, dtype=np.uint64)
    hc = lu.ring_hists(ref, small, *C).sum(axis=0, dtype=np.uint64)
    return SimpleNamespace(cfg=cfg, w0=w0, batch=batch, ids=ids, B=B, C=C,
                           want=rank(hb, hc, ids, BOUND_S, SELECT_K, PPM3))
