"""Service overlap over the window ring (sa_window_overlap): the cases'
workloads and their references, shared by tests/test_window_overlap_host.py
(what the inputs can catch, on the oracle alone) and
tests/test_gpu_window_overlap.py (the kernels).

The range cases of tests/range_util.py put one trace on each span, so every
pair of services there is disjoint.  Here a trace visits several services, and
its spans end in windows drawn independently over the ring: a trace two
services share often meets them in different windows, so pairing per window
cannot stand in for pairing the merged arrays.

Planted structure (engines of 8 services or more; ids in PLANT):

  EMPTY       no span at all: all-zero registers, the linear-counting branch
  SAME        two services on exactly the same traces
  APART       two services with no trace in common
  SUB, SUP    every trace of SUB also visits SUP, which has more of its own
  the rest    every trace visits a run of 1..8 consecutive ids of the rest:
              neighbours share most of their traces, ids 8 apart none

Engines of 2 or 3 services take the runs alone (p18: a quarter of the traces
on each service only, half on both).

Cases (a config, the steps [(ring base, batch)], the final base, the ranges):

  p4        hll_p 4, 3 services, 2 windows: a service is one 16-byte word
  p18       hll_p 18, 2 services, 2 windows, 233,000 traces, half on both
            services, 350,000 spans: the union leaves 2^18 exp(-233,000 /
            2^18) = 107,000 zero registers, so a bin passes 65,535
  p8x64     hll_p 8, 64 services, 4 windows: every one of the 2,016 pairs
  p14x200   the default hll_p, 200 services, 4 windows (selections SEL5, SEL9)
  moved     hll_p 10, 12 services, 4 windows: a batch at w0, the base advanced
            by 3 (slots cleared and reused), a batch over the new ring; every
            first <= last of the ring
  row:<r>   ring_binned and ring_dense of geometry_util.RING_ROWS (2 services)

The reference is pyoracle.Oracle fed, per batch, the spans whose end lay in the
ring as it stood (range_util's rule), its windows max-merged as
range_util.merged does, then per pair np.maximum, np.bincount(minlength=64),
hll_estimate_hist and shared = max(0, (d_i + d_j) - union).  truth() gives the
true set sizes from the trace ids.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import pyoracle
from geometry_util import RING_ROWS, config_of, key_pool, ring_start
from range_util import merged
from ring_util import in_ring
from spanagg import Config, SpanBatch, hll_estimate_hist, pack_meta

BINS = 64
PLANT = SimpleNamespace(EMPTY=0, SAME=(1, 2), APART=(3, 4), SUB=5, SUP=6, REST=7)
SEL5 = (150, 2, 1, 77, 0)
SEL9 = (6, 199, 5, 3, 120, 121, 4, 64, 122)
ROWS = ("ring_binned", "ring_dense")
CONFIGS = dict(p4=Config(key_capacity=1000, hll_p=4, n_services=3, n_windows=2),
               p18=Config(key_capacity=1000, hll_p=18, n_services=2, n_windows=2),
               p8x64=Config(key_capacity=1000, hll_p=8, n_services=64, n_windows=4),
               p14x200=Config(key_capacity=1000, n_services=200, n_windows=4),
               moved=Config(key_capacity=1000, hll_p=10, n_services=12, n_windows=4))
PER_SERVICE = 1500  # traces a service of the rest sees, about
P18_TRACES = 233_000
CASES = list(CONFIGS) + [f"row:{r}" for r in ROWS]


def pair_index(i, j, n):
    assert 0 <= i < j < n
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def _visits(rng, S, per_service):
    """(trace number, service) of every visit, traces numbered from 0."""
    if S < 8:
        lo, planted = 0, []
    else:
        lo = PLANT.REST
        n = per_service
        same = np.arange(n)
        apart_a, apart_b = np.arange(n, 2 * n), np.arange(2 * n, 3 * n)
        sup = np.arange(3 * n, 5 * n)
        sub = sup[: n // 2]
        planted = [(same, PLANT.SAME[0]), (same, PLANT.SAME[1]), (apart_a, PLANT.APART[0]),
                   (apart_b, PLANT.APART[1]), (sub, PLANT.SUB), (sup, PLANT.SUP)]
    t0 = 0 if not planted else 5 * per_service
    R = S - lo
    n_runs = max(R * per_service * 2 // 9, 64)  # a run is 4.5 services long on average
    length = rng.integers(1, 9, n_runs)
    start = rng.integers(0, R, n_runs)
    tr = np.repeat(np.arange(t0, t0 + n_runs), length)
    off = np.concatenate([np.arange(k) for k in length])
    svc = lo + np.repeat(start, length) + off
    keep = svc < S
    cols = [(tr[keep], svc[keep])] + [(t, np.full(len(t), s)) for t, s in planted]
    return np.concatenate([c[0] for c in cols]), np.concatenate([c[1] for c in cols]).astype(np.uint32)


def make_batch(rng, cfg, w0, n_keys, per_service=PER_SERVICE, p18=False) -> SpanBatch:
    """One span per visit (every fourth visit a second one), ends uniform over
    the ring from w0 and independent of the trace: a trace's spans lie in
    different windows.  Valid services and windows only; a fifth ERROR."""
    S, W, wns = cfg.n_services, cfg.n_windows, cfg.window_ns
    if p18:
        assert S == 2
        q = P18_TRACES // 4
        tr = np.concatenate([np.arange(0, 3 * q), np.arange(q, 4 * q)])  # [0, q) svc 0 only, [3q, 4q) svc 1 only
        svc = np.concatenate([np.zeros(3 * q, np.uint32), np.ones(3 * q, np.uint32)])
    else:
        tr, svc = _visits(rng, S, per_service)
    twice = np.flatnonzero(rng.random(len(tr)) < 0.25)
    tr, svc = np.concatenate([tr, tr[twice]]), np.concatenate([svc, svc[twice]])
    order = rng.permutation(len(tr))
    tr, svc = tr[order], svc[order]
    n, nt = len(tr), int(tr.max()) + 1
    ids0, ids1 = rng.integers(0, 2**64, nt, dtype=np.uint64), rng.integers(0, 2**64, nt, dtype=np.uint64)
    end = np.uint64(w0 * wns) + rng.integers(0, W * wns, n, dtype=np.uint64)
    start = end - rng.integers(1, 50_000_000, n, dtype=np.uint64)
    key = key_pool(n_keys)[rng.integers(0, n_keys, n)]
    status = np.where(rng.random(n) < 0.2, 2, 1).astype(np.uint32)
    return SpanBatch(key, start, end, ids0[tr], ids1[tr], pack_meta(svc, rng.integers(0, 6, n), status))


@functools.lru_cache(maxsize=3)
def case(name):
    rng = np.random.default_rng(zlib.crc32(("overlap:" + name).encode()))
    if name.startswith("row:"):
        row = name[4:]
        cfg, nk = config_of(row), RING_ROWS[row]["n_keys"]
    else:
        row, cfg, nk = None, CONFIGS[name], 700
    w0, W = ring_start(cfg), cfg.n_windows
    per = 200 if name == "p4" else 3000 if row else PER_SERVICE
    steps, base = [(w0, make_batch(rng, cfg, w0, nk, per, p18=name == "p18"))], w0
    if name == "moved":
        base = w0 + 3
        steps.append((base, make_batch(rng, cfg, base, nk, per)))
        ranges = [(a, b) for a in range(base, base + W) for b in range(a, base + W)]
    else:
        ranges = [(base, base + W - 1)]
    return SimpleNamespace(name=name, cfg=cfg, steps=steps, base=base, ranges=ranges, row=row)


@functools.lru_cache(maxsize=3)
def reference(name):
    """The oracle's registers [n_services, 2^p] of every window of the case's
    final ring (zeros for a window no span touched), as range_util.reference
    pairs them with the cells."""
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def pairs_of(hll, p):
    """From registers [n, 2^p] (already merged, already selected): what
    window_overlap must return for them."""
    n = len(hll)
    hist = np.stack([np.bincount(row, minlength=BINS) for row in hll]).astype(np.uint32)
    distinct = np.array([hll_estimate_hist(h, p) for h in hist])
    npairs = n * (n - 1) // 2
    pair_hist = np.zeros((npairs, BINS), np.uint32)
    union, shared = np.diag(distinct), np.diag(distinct)
    for i in range(n):
        for j in range(i + 1, n):
            row = np.bincount(np.maximum(hll[i], hll[j]), minlength=BINS).astype(np.uint32)
            pair_hist[pair_index(i, j, n)] = row
            union[i, j] = union[j, i] = hll_estimate_hist(row, p)
            shared[i, j] = shared[j, i] = max(0.0, (distinct[i] + distinct[j]) - union[i, j])
    return SimpleNamespace(hist=hist, distinct=distinct, pair_hist=pair_hist, union=union, shared=shared)


def expected(windows, wins, services, p):
    """The reference of window_overlap over the window ids `wins` for the
    service ids `services` (in that order): merge first, then pair."""
    hll = merged(windows, wins, ()).hll[np.asarray(services, dtype=np.int64)]
    want = pairs_of(hll, p)
    want.services = np.asarray(services, dtype=np.uint32)
    return want


def strongest(shared, services, k):
    n = len(services)
    pairs = sorted(((i, j) for i in range(n) for j in range(i + 1, n)), key=lambda ij: (-float(shared[ij]), ij))
    return [(int(services[i]), int(services[j]), float(shared[i, j])) for i, j in pairs[:k]]


def truth(c, first, last):
    """The true trace sets: per service the set of (w0, w1) trace ids with a
    span whose end lies in windows first..last of the final ring (and lay in
    the ring when its batch went in)."""
    cfg = c.cfg
    sets = [set() for _ in range(cfg.n_services)]
    for base, batch in c.steps:
        b = in_ring(batch, cfg, base)
        w = b.end_ns // np.uint64(cfg.window_ns)
        keep = (w >= max(first, c.base)) & (w <= last)
        svc = (b.meta & np.uint32(0xFFFF))[keep]
        ids = np.stack([b.trace_w0[keep], b.trace_w1[keep]], axis=1)
        for s in np.unique(svc):
            sets[int(s)].update(map(tuple, ids[svc == s].tolist()))
    return sets


def assert_overlap_equal(r, want, cfg, what):
    """An OverlapResult against expected(): bit-exact, every row summing to
    2^p, and union / shared / strongest recomputed from the returned
    histograms."""
    p, n = cfg.hll_p, len(want.services)
    assert np.array_equal(r.services, want.services) and r.services.dtype == np.uint32, ("services", what)
    assert r.p == p and r.hist.shape == (n, BINS) and r.pair_hist.shape == (n * (n - 1) // 2, BINS), what
    assert np.array_equal(r.hist, want.hist), ("hist", what)
    assert np.array_equal(r.pair_hist, want.pair_hist), ("pair_hist", what)
    assert (r.hist.sum(axis=1) == 1 << p).all() and (r.pair_hist.sum(axis=1) == 1 << p).all(), what
    assert [float(d) for d in r.distinct] == [hll_estimate_hist(h, p) for h in r.hist], ("distinct", what)
    union, shared = np.diag(r.distinct), np.diag(r.distinct)
    for i in range(n):
        for j in range(i + 1, n):
            union[i, j] = union[j, i] = hll_estimate_hist(r.pair_hist[pair_index(i, j, n)], p)
            shared[i, j] = shared[j, i] = max(0.0, (float(r.distinct[i]) + float(r.distinct[j])) - union[i, j])
            assert r.pair_index(i, j) == r.pair_index(j, i) == pair_index(i, j, n)
    assert np.array_equal(r.union, union) and np.array_equal(r.union, want.union), ("union", what)
    assert np.array_equal(r.shared, shared) and np.array_equal(r.shared, want.shared), ("shared", what)
    for k in (1, 10, n * n):
        assert r.strongest(k) == strongest(shared, r.services, k), ("strongest", k, what)
