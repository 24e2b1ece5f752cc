"""Window-range queries (sa_window_range): the cases' workloads and their
oracle references, shared by tests/test_window_range_host.py (what the inputs
can catch, on the oracle alone) and tests/test_gpu_window_range.py (the
kernels).

A case is a config, the batches with the ring base each goes in under, the
keys of the point queries and the (first, last) ranges to ask for:

  full:<row>   every row of geometry_util.RING_ROWS: one batch over the ring
               at w0, the whole ring as one range
  moved:<row>  ring_512 (4 windows) and ring_1024_noerr (32): a batch at w0,
               the base advanced by 3 (slots are cleared and reused), a batch
               over the new ring.  ring_512: every first <= last of the ring;
               ring_1024_noerr: the ranges of 1, 2, 31 and 32 windows around
               the step from slot n_windows - 1 to slot 0
  p4, p18      the extremes of hll_p on two windows: 3 services of 16
               registers (one thread's load each), and one service of 2^18
               registers
  group        synth.generate_c2(400_003) on a 16-window ring, five windows

Batches hold about 24 spans per register of the ring (the ring rows' fill), at
least 60,000, one trace per span: with traces shared across the ring a window
adds nothing to the other windows' maxima, and a range short of one window
would not show.  p18 takes 350,003 spans: with n distinct traces in a ring of
m = 2^18 registers the merged array's zero bin holds m * exp(-n / m) registers,
70,000 at n = 343,000 (what stays of the batch inside the ring), so a bin's
count passes 65,535 -- the bins for 1 and 2 top out at m / 4 = 65,536 for any n,
and 400,000 spans leave 58,000 zeros.

Keys: the first 200 of the row's key pool (its 8 hot keys among them), 99 ids
never ingested, and key 0.

The reference is pyoracle.Oracle fed, per batch, the spans whose end lay in
the ring as it stood: registers max-merged over the range's windows, their
histogram per service, the cells summed as u64, sketch.cms_query on the sum.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import pyoracle
from geometry_util import RING_ROWS, config_of, key_pool, make_batch, ring_start
from ring_util import in_ring
from spanagg import Config
from spanagg.sketch import cms_query
from spanagg.synth import generate_c2

BINS = 64
MOVED = ("ring_512", "ring_1024_noerr")
EXTREMES = dict(p4=(Config(key_capacity=1000, hll_p=4, n_services=3, n_windows=2), 60_000),
                p18=(Config(key_capacity=1000, hll_p=18, n_services=1, n_windows=2), 350_003))
CASES = [f"full:{row}" for row in RING_ROWS] + [f"moved:{row}" for row in MOVED] + list(EXTREMES) + ["group"]
GROUP_SPANS, GROUP_SEED, GROUP_WINDOWS = 400_003, 21, 16


def query_keys(pool, seed) -> np.ndarray:
    """200 keys of the pool, 99 ids outside it, key 0."""
    rng = np.random.default_rng([seed, 0xAB5E])
    fresh = rng.integers(1, 2**64, 400, dtype=np.uint64)
    fresh = fresh[~np.isin(fresh, pool)][:99]
    keys = np.concatenate([pool[:200], fresh, np.zeros(1, np.uint64)])
    assert len(keys) == 300
    return keys


def _around_wrap(base, W):
    """Ranges of 1, 2, W - 1 and W windows of the ring at `base` around the
    step from slot W - 1 to slot 0."""
    wc = next(w for w in range(base, base + W) if w & (W - 1) == W - 1)
    assert base <= wc < base + W - 1, "the ring must wrap inside"
    return [(wc, wc), (wc + 1, wc + 1), (wc, wc + 1), (base, base + W - 2), (base + 1, base + W - 1),
            (base, base + W - 1)]


@functools.lru_cache(maxsize=2)
def case(name):
    """The case's config, steps [(ring base, batch)], query keys, ranges and
    final ring base."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "group":
        wl = generate_c2(GROUP_SPANS, seed=GROUP_SEED)
        cfg = Config(n_services=wl.n_services, n_windows=GROUP_WINDOWS)
        base = wl.first_window
        keys = query_keys(wl.key_hashes[2::3], 7)  # the ERROR series
        return SimpleNamespace(name=name, cfg=cfg, steps=[(base, wl.batch)], keys=keys, base=base,
                               ranges=[(base + 1, base + 5)], row=None)
    kind, _, row = name.partition(":")
    if name in EXTREMES:
        cfg, n = EXTREMES[name]
        nk, row = 700, None
    else:
        cfg, r = config_of(row), RING_ROWS[row]
        nk = r["n_keys"]
        n = max(r["fill"] * ((cfg.n_windows * cfg.n_services) << cfg.hll_p), 60_000)
    w0, W = ring_start(cfg), cfg.n_windows
    steps = [(w0, make_batch(rng, n, cfg, nk, w0=w0, distinct_traces=True))]
    base = w0
    if kind == "moved":
        base = w0 + 3
        steps.append((base, make_batch(rng, n, cfg, nk, w0=base, distinct_traces=True)))
        ranges = ([(a, b) for a in range(base, base + W) for b in range(a, base + W)] if row == "ring_512"
                  else _around_wrap(base, W))
    else:
        ranges = [(base, base + W - 1)]
    return SimpleNamespace(name=name, cfg=cfg, steps=steps, keys=query_keys(key_pool(nk), nk), base=base,
                           ranges=ranges, row=row)


@functools.lru_cache(maxsize=2)
def reference(name):
    """The oracle's (registers, cells) of every window of the case's final
    ring (zeros for a window no span touched)."""
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def merged(windows, wins, keys):
    """What a range query over the window ids `wins` must return."""
    hll = np.maximum.reduce([windows[w][0] for w in wins])
    cms = np.sum([windows[w][1].astype(np.uint64) for w in wins], axis=0, dtype=np.uint64)
    hist = np.stack([np.bincount(row, minlength=BINS) for row in hll]).astype(np.uint32)
    errors = np.array([cms_query(cms, int(k)) for k in keys], dtype=np.uint64)
    return SimpleNamespace(hist=hist, hll=hll, cms=cms, errors=errors)


def unmasked(first, last, W):
    """The windows a walk without the ring mask still reads inside the ring:
    slots (first & (W - 1)) + k for k = 0 .. last - first, those below W.
    None when the range does not wrap."""
    s0, n = first & (W - 1), last - first + 1
    return [first + k for k in range(n) if s0 + k < W] if s0 + n > W else None


def assert_range_equal(r, want, cfg, what):
    """A RangeResult asked for with both flags against merged()'s reference:
    bit-exact, and the estimates are the histogram's."""
    from spanagg import hll_estimate_hist
    assert np.array_equal(r.hist, want.hist), ("hist", what)
    assert np.array_equal(r.hll, want.hll), ("hll", what)
    assert r.cms.dtype == np.uint64 and np.array_equal(r.cms, want.cms), ("cms", what)
    assert np.array_equal(r.errors, want.errors), ("errors", what)
    assert (r.hist.sum(axis=1) == 1 << cfg.hll_p).all(), what
    assert [float(d) for d in r.distinct] == [hll_estimate_hist(h, cfg.hll_p) for h in r.hist], ("distinct", what)
