"""Movers over the window ring (sa_window_movers): the cases' workloads and
their oracle answers, shared by tests/test_window_movers_host.py (what the
inputs can catch, on the oracle alone) and tests/test_gpu_window_movers.py (the
kernels).

Cases of top_util and range_util are taken as they are (full:<row>,
moved:<row>, ties_small, ties_binned, the cell sizes, group).  The case of this
file:

  planted   the ring_512 config (4 windows), 60,000 spans on 560 keys with 1 in
            20 ERROR, and an incident: every span of three of the hot keys that
            ends in the ring's last window is ERROR.  Baseline: the first three
            windows; current: the last.

The reference: the oracle's cells of each range's windows summed as u64
(top_util.cells), the candidates the distinct non-zero key_hash of the batches
ingested, the estimates sketch.cms_query's in both sums (top_util.estimates),
score = current * n_base - baseline * n_cur in int64 (negated for the fall), the
order score descending then key ascending.  movers() is that vectorised;
tests/test_window_movers_host.py holds it against sketch.movers.
"""
import functools
from types import SimpleNamespace

import numpy as np

import pyoracle
import top_util
from geometry_util import config_of, key_pool, make_batch, ring_start
from ring_util import in_ring
from top_util import candidates, cells, estimates  # noqa: F401  (the tests take them from here)

PLANTED_SEED, PLANTED_KEYS, PLANTED_SPANS, PLANTED_AT = 5, 560, 60_000, (1, 4, 6)
ERROR = np.uint32(2 << 19)  # status.code 2 in meta bits 19-20
STATUS_MASK = np.uint32(3 << 19)


def planted_keys() -> np.ndarray:
    return key_pool(PLANTED_KEYS)[list(PLANTED_AT)]


@functools.lru_cache(maxsize=2)
def case(name):
    """top_util.case's shape: cfg, steps [(ring base, batch)], base, ranges, row."""
    if name != "planted":
        return top_util.case(name)
    cfg = config_of("ring_512")
    w0, W = ring_start(cfg), cfg.n_windows
    rng = np.random.default_rng(PLANTED_SEED)
    batch = make_batch(rng, PLANTED_SPANS, cfg, PLANTED_KEYS, error_share=0.05, distinct_traces=True)
    last = (batch.end_ns // np.uint64(cfg.window_ns)) == np.uint64(w0 + W - 1)
    hit = last & np.isin(batch.key_hash, planted_keys())
    batch.meta[hit] = (batch.meta[hit] & ~STATUS_MASK) | ERROR
    return SimpleNamespace(name=name, cfg=cfg, steps=[(w0, batch)], keys=key_pool(PLANTED_KEYS)[:0], base=w0,
                           ranges=[(w0, w0 + W - 1)], row="ring_512")


@functools.lru_cache(maxsize=2)
def reference(name):
    """top_util.reference: the oracle's (registers, cells) of every window of the final ring."""
    if name != "planted":
        return top_util.reference(name)
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def split(c):
    """The default (baseline, current) ranges of the case's full ring of W
    windows: its first W // 2 and its last W // 2 windows (W == 2: one window
    each; W == 1: both the one window)."""
    W, a = c.cfg.n_windows, c.base
    if W == 1:
        return (a, a), (a, a)
    if c.name == "planted":
        return (a, a + W - 2), (a + W - 1, a + W - 1)
    return (a, a + W // 2 - 1), (a + W - W // 2, a + W - 1)


def scores(cms_base, cms_cur, n_base, n_cur, cand, fall=False):
    """(baseline, current, score) of every candidate: u64, u64, int64."""
    b, c = estimates(cms_base, cand), estimates(cms_cur, cand)
    s = c.astype(np.int64) * np.int64(n_base) - b.astype(np.int64) * np.int64(n_cur)
    return b, c, -s if fall else s


def ranked(score, cand, min_score=1, reverse_ties=False):
    """The positions of the candidates with score >= max(min_score, 1), by
    score descending then key ascending (reverse_ties: descending)."""
    cand = np.asarray(cand, dtype=np.uint64)
    floor = max(int(min_score), 1)
    keep = np.flatnonzero(score >= floor) if floor < 2**63 else np.zeros(0, np.int64)
    tie = top_util.M64 - cand[keep] if reverse_ties else cand[keep]
    return keep[np.lexsort((tie, -score[keep]))]


def movers(windows, base, cur, cand, k, min_score=1, fall=False):
    """What sa_window_movers must return over the oracle's `windows` for the
    ranges base = (first, last) and cur with the candidates `cand` (distinct,
    non-zero)."""
    cand = np.asarray(cand, dtype=np.uint64)
    cb, cc = cells(windows, *base), cells(windows, *cur)
    b, c, s = scores(cb, cc, base[1] - base[0] + 1, cur[1] - cur[0] + 1, cand, fall)
    order = ranked(s, cand, min_score)
    top = order[:k]
    return SimpleNamespace(keys=cand[top], score=s[top], baseline=b[top], current=c[top], n_resident=len(cand),
                           n_matched=len(order), error_spans_base=int(cb[0].sum(dtype=np.uint64)),
                           error_spans_cur=int(cc[0].sum(dtype=np.uint64)))


def items(m):
    return [(int(k), int(s), int(b), int(c)) for k, s, b, c in zip(m.keys, m.score, m.baseline, m.current)]


def assert_movers_equal(r, want, what):
    """A MoversResult against movers()'s reference: every list and counter, bit for bit."""
    assert r.keys.dtype == r.baseline.dtype == r.current.dtype == np.uint64 and r.score.dtype == np.int64, what
    assert np.array_equal(r.keys, want.keys), ("keys", what)
    assert np.array_equal(r.score, want.score), ("score", what)
    assert np.array_equal(r.baseline, want.baseline), ("baseline", what)
    assert np.array_equal(r.current, want.current), ("current", what)
    got = (r.n_resident, r.n_matched, r.error_spans_base, r.error_spans_cur)
    assert got == (want.n_resident, want.n_matched, want.error_spans_base, want.error_spans_cur), ("counters", what, got)
