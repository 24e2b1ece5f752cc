"""Sliding series over the window ring (sa_window_series): the cases, the
(first, last, width) series asked of each and their oracle references, shared
by tests/test_window_series_host.py (what the inputs can catch, on the oracle
alone) and tests/test_gpu_window_series.py (the kernels).

The cases are range_util's (full:<row> for every row of RING_ROWS, the two
moved rings, p4 and p18) and one more:

  long   Config(key_capacity=800, hll_p=6, n_services=3, n_windows=256): a
         batch over the ring at w0, the base advanced by 5 (slots are cleared
         and reused: every series that reaches the last five windows passes the
         slot wrap), a batch over the new ring.  24 spans per register of the
         ring a step (1,179,648), 30 % of them ERROR, one trace per span.
         At p = 6 a slot holds 192 registers, and of a span of w windows a
         given window holds a register's strict maximum in about 192 x 0.7 / w
         of them: from w ~ 64 a window more or less would often show in no
         histogram.  So the second batch also carries one marker span per
         window: window base + k raises register k mod 192 of the slot to 41
         (k < 192) or 40 (k >= 192) -- above anything 2.4 M random traces
         reach, and the earlier of two windows that share a register holds the
         larger value, so in every span the first window holds a strict
         maximum and the window before the span exceeds it.  The marker's
         trace id is built from the wanted hash (hll_util.trace_with_hash: the 16-byte
         xxh64 run backwards).

  wide512  Config(key_capacity=800, hll_p=5, n_services=20, n_windows=512): one
         batch of 4 spans per register of the ring (1,310,720) and the marker
         spans (640 registers a slot: every window its own, all 41).  A slot
         is 40 register columns of two a service: at widths over 256 the
         kernel's tiles are 32 columns -- 16 services, then 8 columns of 4.

Output t of a series of width w is what a range query over the windows
t - w + 1 .. t returns: range_util.merged().  series() computes the same for a
whole series at once -- the registers' maxima per output, and the errors from
prefix sums over the windows' cells at the keys' columns (columns()); the host
test holds it against merged() on the first, last and a seam output of every
series, so the GPU test may rely on it.

PLANS lists every series the GPU test asks for; the host test walks the same
list.  The kernel cuts a series into blocks of `width` outputs (block j:
outputs j * width ..), so outputs j * width - 1, j * width and j * width + 1
are the block seams (checked()).
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import range_util
from geometry_util import RING_ROWS, key_pool, make_batch, ring_start
from hll_util import trace_with_hash
from spanagg import Config
from spanagg.sketch import CMS_SEEDS

BINS = range_util.BINS
LONG_CFG = Config(key_capacity=800, hll_p=6, n_services=3, n_windows=256)
LONG_KEYS, LONG_FILL, LONG_STEP = 560, 24, 5
# The kernel keeps a block's suffix maxima in a 32 KiB LDS stash.  Tiles of 64
# columns (1 KiB a window) hold a whole block up to width 32: two reads a
# window.  From 33 a block goes in chunks (16 windows, and the maxima of the
# later chunks): three reads, 64 columns up to width 256, 32 columns up to
# 1,024, 16 up to 4,096.  32 | 33 is the bound `long` straddles; 257 needs
# more than `long`'s 256 windows: the `wide512` case.
LONG_WIDTHS = (1, 7, 32, 33, 64, 100, 128, 129, 255, 256)
WIDE_CFG = Config(key_capacity=800, hll_p=5, n_services=20, n_windows=512)
WIDE_FILL, WIDE_WIDTHS = 4, (256, 257, 512)
NOERR_WIDTHS = (1, 2, 3, 5, 8, 16, 31, 32)


def long_markers(cfg, base):
    """One span per window base + k of the ring: register k mod regs of the
    slot (service and index; regs = n_services * 2^p, 192 for `long`) raised
    to 41, or 40 for k >= regs."""
    from spanagg import SpanBatch, pack_meta
    p, W, m = cfg.hll_p, cfg.n_windows, 1 << cfg.hll_p
    regs = cfg.n_services * m
    k = np.arange(W)
    q, rho = k % regs, np.where(k < regs, 41, 40)
    t0 = np.arange(1, W + 1, dtype=np.uint64) * np.uint64(0x1234567)
    t1 = np.array([trace_with_hash((int(qi % m) << (64 - p)) | (1 << (64 - p - int(h))) | 0x155, int(a))
                   for qi, h, a in zip(q, rho, t0)], dtype=np.uint64)
    end = (np.uint64(base) + k.astype(np.uint64)) * np.uint64(cfg.window_ns) + np.uint64(4321)
    return SpanBatch(key_pool(LONG_KEYS)[k % 8], end - np.uint64(1000), end, t0, t1,
                     pack_meta(q // m, np.ones(W, np.uint32), np.zeros(W, np.uint32)))


def _long_case():
    from geometry_util import concat
    rng = np.random.default_rng(zlib.crc32(b"long"))
    cfg = LONG_CFG
    n = LONG_FILL * ((cfg.n_windows * cfg.n_services) << cfg.hll_p)
    w0 = ring_start(cfg)
    base = w0 + LONG_STEP
    steps = [(w0, make_batch(rng, n, cfg, LONG_KEYS, w0=w0, distinct_traces=True)),
             (base, concat([make_batch(rng, n, cfg, LONG_KEYS, w0=base, distinct_traces=True),
                            long_markers(cfg, base)]))]
    return SimpleNamespace(name="long", cfg=cfg, steps=steps, keys=range_util.query_keys(key_pool(LONG_KEYS), LONG_KEYS),
                           base=base, ranges=[], row=None)


def _wide_case():
    from geometry_util import concat
    rng = np.random.default_rng(zlib.crc32(b"wide512"))
    cfg = WIDE_CFG
    n = WIDE_FILL * ((cfg.n_windows * cfg.n_services) << cfg.hll_p)
    base = ring_start(cfg)
    steps = [(base, concat([make_batch(rng, n, cfg, LONG_KEYS, w0=base, distinct_traces=True), long_markers(cfg, base)]))]
    return SimpleNamespace(name="wide512", cfg=cfg, steps=steps,
                           keys=range_util.query_keys(key_pool(LONG_KEYS), LONG_KEYS), base=base, ranges=[], row=None)


OWN = {"long": _long_case, "wide512": _wide_case}


@functools.lru_cache(maxsize=2)
def case(name):
    """range_util.case(name), or one of the cases built here: config, steps
    [(ring base, batch)], query keys and final ring base."""
    return OWN[name]() if name in OWN else range_util.case(name)


@functools.lru_cache(maxsize=2)
def reference(name):
    """The oracle's (registers, cells) of every window of the case's final ring."""
    if name not in OWN:
        return range_util.reference(name)
    import pyoracle
    from ring_util import in_ring
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def _splitmix64(x):
    with np.errstate(over="ignore"):
        z = x + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def columns(keys, d, w):
    """[d][n_keys] the count-min column of every key in every row (sketch.cms_query's)."""
    k = np.asarray(keys, dtype=np.uint64)
    shift = np.uint64(64 - (int(w).bit_length() - 1))
    return np.stack([_splitmix64(k ^ np.uint64(CMS_SEEDS[r])) >> shift for r in range(d)]).astype(np.int64)


def hist_of(windows, wins):
    """[n_services][64] the histogram of the registers max-merged over the window ids `wins`."""
    hll = np.maximum.reduce([windows[w][0] for w in wins])
    return np.stack([np.bincount(row, minlength=BINS) for row in hll]).astype(np.uint32)


def series(windows, first, last, width, keys):
    """What sa_window_series(first, last, width, keys) must return: hist
    [n_out][S][64], error_spans [n_out], errors [n_out][n_keys]."""
    a, n_out = first - width + 1, last - first + 1
    ins = range(a, last + 1)
    hist = np.stack([hist_of(windows, range(t - width + 1, t + 1)) for t in range(first, last + 1)])
    cms0 = windows[a][1]
    d, w = cms0.shape
    cols = columns(keys, d, w)
    # cells[k][r][i]: window a + k's cell of key i in row r, then prefix sums over k
    cells = np.stack([windows[t][1][np.arange(d)[:, None], cols].astype(np.uint64) for t in ins])
    pre = np.concatenate([np.zeros((1,) + cells.shape[1:], np.uint64), np.cumsum(cells, axis=0, dtype=np.uint64)])
    errors = (pre[width:] - pre[:-width]).min(axis=1) if len(cols[0]) else np.zeros((n_out, 0), np.uint64)
    row0 = np.array([int(windows[t][1][0].astype(np.uint64).sum()) for t in ins], dtype=np.uint64)
    pre0 = np.concatenate([np.zeros(1, np.uint64), np.cumsum(row0, dtype=np.uint64)])
    assert errors.shape == (n_out, len(cols[0])) and hist.shape[0] == n_out
    return SimpleNamespace(hist=hist, errors=errors.astype(np.uint64), error_spans=pre0[width:] - pre0[:-width])


@functools.lru_cache(maxsize=64)
def expected(name, first, last, width):
    """series() of the case's reference windows and keys (computed once, shared)."""
    r = series(reference(name), first, last, width, case(name).keys)
    for arr in (r.hist, r.errors, r.error_spans):
        arr.setflags(write=False)
    return r


def checked(first, last, width, W):
    """Outputs (window ids) a host check looks at: the first, the last, the
    block seams j * width - 1, j * width, j * width + 1 (at most the first three
    and the last blocks' when there are many), and the outputs whose span
    starts at ring slot W - 1, W - 2 (it passes the slot wrap)."""
    n_out = last - first + 1
    blocks = list(range(1, (n_out + width - 1) // width))
    if len(blocks) > 6:
        blocks = blocks[:3] + blocks[-3:]
    outs = {0, n_out - 1} | {j * width + k for j in blocks for k in (-1, 0, 1)}
    ts = {first + o for o in outs if 0 <= o < n_out}
    ts |= {t for t in range(first, last + 1) if width > 1 and (t - width + 1) & (W - 1) in (W - 1, W - 2)}
    return sorted(ts)


def _largest(base, W, width):
    return (base + width - 1, base + W - 1, width)


def _plans():
    plans = {}
    for row in RING_ROWS:
        name = f"full:{row}"
        cfg = range_util.config_of(row)
        base, W = ring_start(cfg), cfg.n_windows
        p = [_largest(base, W, 1)]
        if W > 1:
            p.append(_largest(base, W, W))
        if W >= 4:
            p.append(_largest(base, W, 2))
        plans[name] = p
    cfg = range_util.config_of("ring_512")
    base, W = ring_start(cfg) + 3, cfg.n_windows
    plans["moved:ring_512"] = [(f, l, w) for w in range(1, W + 1) for f in range(base + w - 1, base + W)
                               for l in range(f, base + W)]
    cfg = range_util.config_of("ring_1024_noerr")
    base, W = ring_start(cfg) + 3, cfg.n_windows
    plans["moved:ring_1024_noerr"] = ([_largest(base, W, w) for w in NOERR_WIDTHS]
                                      + [(base + 4, base + 4 + n - 1, 5) for n in (4, 5, 6)])
    base, W = ring_start(LONG_CFG) + LONG_STEP, LONG_CFG.n_windows
    plans["long"] = [_largest(base, W, w) for w in LONG_WIDTHS]
    base, W = ring_start(WIDE_CFG), WIDE_CFG.n_windows
    plans["wide512"] = [_largest(base, W, w) for w in WIDE_WIDTHS]
    for name, (cfg, _) in range_util.EXTREMES.items():
        base = ring_start(cfg)
        plans[name] = [_largest(base, 2, 1), _largest(base, 2, 2)]
    return plans


PLANS = _plans()


def assert_series_equal(r, want, cfg, first, last, width, what):
    """A SeriesResult against series()'s reference: bit-exact, and the
    estimates are the histograms'."""
    from spanagg import hll_estimate_hist
    n_out = last - first + 1
    assert (r.first, r.last, r.width) == (first, last, width), what
    assert r.hist.shape == (n_out, cfg.n_services, BINS) and r.hist.dtype == np.uint32, what
    assert np.array_equal(r.hist, want.hist), ("hist", what, np.argwhere((r.hist != want.hist).any(axis=(1, 2))).ravel()[:8])
    assert r.errors.shape == want.errors.shape and r.errors.dtype == np.uint64, what
    assert np.array_equal(r.errors, want.errors), ("errors", what)
    assert r.error_spans.dtype == np.uint64 and np.array_equal(r.error_spans, want.error_spans), ("error_spans", what)
    assert (r.hist.sum(axis=2) == 1 << cfg.hll_p).all(), what
    assert r.distinct.shape == (n_out, cfg.n_services), what
    est = {}  # (many rows repeat on small rings; the estimator is a pure function of the row)
    for i in range(n_out):
        for s in range(cfg.n_services):
            key = r.hist[i, s].tobytes()
            if key not in est:
                est[key] = hll_estimate_hist(r.hist[i, s], cfg.hll_p)
            assert float(r.distinct[i, s]) == est[key], ("distinct", what, i, s)
