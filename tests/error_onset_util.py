"""Error onset over the window ring (sa_window_error_onset): the cases'
workloads and their oracle answers, shared by
tests/test_window_error_onset_host.py (the rule and what the inputs can catch,
on the oracle alone) and tests/test_gpu_window_error_onset.py (the kernels).

Cases of movers_util, top_util and range_util are taken as they are
(full:<row>, moved:<row>, ties_binned, group).  The cases of this file:

  steps      a default ring of 8 windows (count-min 4 x 2,048), six series
             with hand-written ERROR counts per window (STEPS): errors only
             in the last window, only in the first, a run of empty windows
             before the onset, two splits that tie, a constant series, and
             one that never fails
  collide    the default ring with a count-min of 2 x 4: K fails once a
             window, X shares K's column in row 0 only and fails early, Y
             shares K's column in row 1 only and fails late -- so K's "before"
             is row 1's and its "after" is row 0's
  all_tied   count-min 1 x 2, 300 series, one failing series a column with
             the same counts per window: every candidate has the same score
  long128, long1024
             rings of 128 and 1,024 windows (hll_p 4, one service, count-min
             2 x 64), moved so that the range wraps
  binned_w64k, dense_w64k
             the 2^19-slot binned and dense-ids rows with count-min 4 x
             65,536: 2 MiB of summed cells, past what a workgroup stages (the
             rows' own 4 x 2,048 is the bound itself)

The reference: the oracle's cells of each window of the range, the candidates
the distinct non-zero key_hash of the batches ingested, and the rule of
include/spanagg.h restated on numpy arrays (onset());
tests/test_window_error_onset_host.py holds it against sketch.error_onset.
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import movers_util
import pyoracle
from geometry_util import config_of, key_pool, make_batch, ring_start
from ring_util import in_ring
from series_util import columns
from spanagg import Config, SpanBatch, pack_meta
from top_util import candidates  # noqa: F401  (the tests take it from here)

I64_MIN = np.iinfo(np.int64).min

# per series: the ERROR spans of windows 0..7 (every series also has one span that is not an ERROR a window)
STEPS = dict(last=(0, 0, 0, 0, 0, 0, 0, 5), first=(5, 0, 0, 0, 0, 0, 0, 0), gap=(0, 0, 0, 0, 0, 3, 3, 3),
             tie=(1, 0, 0, 0, 0, 1, 0, 2), flat=(2, 2, 2, 2, 2, 2, 2, 2), never=(0, 0, 0, 0, 0, 0, 0, 0))
_SMALL = dict(key_capacity=1000, hll_p=4, n_services=1, n_windows=8)
_LONG = dict(key_capacity=800, hll_p=4, n_services=1, cms_d=2, cms_w=64)


def craft(cfg, w0, rows, seed=0) -> SpanBatch:
    """rows of (key, window offset, ERROR spans, other spans): that many spans
    of service 0 ending inside window w0 + offset, a trace each."""
    key, win, status = [], [], []
    for k, off, n_err, n_ok in rows:
        key += [int(k)] * (n_err + n_ok)
        win += [w0 + off] * (n_err + n_ok)
        status += [2] * n_err + [1] * n_ok
    n = len(key)
    rng = np.random.default_rng([seed, 0xE0])
    end = np.asarray(win, dtype=np.uint64) * np.uint64(cfg.window_ns) + rng.integers(0, cfg.window_ns, n, dtype=np.uint64)
    t0, t1 = rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**64, n, dtype=np.uint64)
    return SpanBatch(np.asarray(key, dtype=np.uint64), end - np.uint64(1000), end, t0, t1,
                     pack_meta(np.zeros(n, np.uint32), np.ones(n, np.uint32), np.asarray(status, dtype=np.uint32)))


def step_keys():
    return dict(zip(STEPS, key_pool(len(STEPS)).tolist()))


def collide_keys(d=2, w=4):
    """(K, X, Y) of key_pool(400): X in K's column in row 0 only, Y in K's column in row 1 only."""
    pool = key_pool(400)
    c = columns(pool, d, w)
    x = next(i for i in range(1, 400) if c[0, i] == c[0, 0] and c[1, i] != c[1, 0])
    y = next(i for i in range(1, 400) if c[1, i] == c[1, 0] and c[0, i] != c[0, 0] and c[0, i] != c[0, x] and c[1, i] != c[1, x])
    return int(pool[0]), int(pool[x]), int(pool[y])


def _own(name):
    if name == "steps":
        cfg = Config(**_SMALL)
        w0 = ring_start(cfg)
        rows = [(k, j, e, 1) for s, k in step_keys().items() for j, e in enumerate(STEPS[s])]
        return cfg, [(w0, craft(cfg, w0, rows))], w0, None
    if name == "collide":
        cfg = Config(cms_d=2, cms_w=4, **_SMALL)
        w0 = ring_start(cfg)
        K, X, Y = collide_keys()
        rows = [(K, j, 1, 0) for j in range(8)] + [(X, j, 10, 0) for j in range(4)] + [(Y, j, 10, 0) for j in range(4, 8)]
        return cfg, [(w0, craft(cfg, w0, rows))], w0, None
    if name == "all_tied":
        cfg = Config(cms_d=1, cms_w=2, **_SMALL)
        w0 = ring_start(cfg)
        pool = key_pool(300)
        col = columns(pool, 1, 2)[0]
        fail = [int(pool[np.flatnonzero(col == c)[0]]) for c in (0, 1)]
        rows = [(k, j, e, 0) for k in fail for j, e in enumerate(STEPS["gap"])] + [(int(k), 3, 0, 1) for k in pool]
        return cfg, [(w0, craft(cfg, w0, rows))], w0, None
    if name in ("long128", "long1024"):
        W = int(name[4:])
        cfg = Config(n_windows=W, **_LONG)
        w0, rng = ring_start(cfg), np.random.default_rng(zlib.crc32(name.encode()))
        base = w0 + W // 2 + 3  # (the first half retires: the ring wraps inside every long range)
        steps = [(w0, make_batch(rng, 40_000, cfg, 300, w0=w0, distinct_traces=True)),
                 (base, make_batch(rng, 40_000, cfg, 300, w0=base, distinct_traces=True))]
        return cfg, steps, base, None
    if name in ("binned_w64k", "dense_w64k"):
        row = "ring_binned" if name == "binned_w64k" else "ring_dense"
        cfg = dataclasses.replace(config_of(row), cms_w=65536)
        w0, rng = ring_start(cfg), np.random.default_rng(zlib.crc32(name.encode()))
        return cfg, [(w0, make_batch(rng, 120_000, cfg, 20_000, w0=w0, distinct_traces=True))], w0, None
    raise KeyError(name)


OWN = ("steps", "collide", "all_tied", "long128", "long1024", "binned_w64k", "dense_w64k")


@functools.lru_cache(maxsize=2)
def case(name):
    """movers_util.case's shape: cfg, steps [(ring base, batch)], base (the final ring's), row."""
    if name not in OWN:
        return movers_util.case(name)
    cfg, steps, base, row = _own(name)
    return SimpleNamespace(name=name, cfg=cfg, steps=steps, base=base, ranges=[(base, base + cfg.n_windows - 1)], row=row)


@functools.lru_cache(maxsize=2)
def reference(name):
    """movers_util.reference: the oracle's (registers, cells) of every window of the final ring."""
    if name not in OWN:
        return movers_util.reference(name)
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def window_cells(windows, first, last) -> np.ndarray:
    """[n][d][w] u64: the cells of windows first..last, one a row."""
    return np.stack([windows[w][1].astype(np.uint64) for w in range(first, last + 1)])


def splits(x, cand, fall=False):
    """Per candidate over the windows' cells x [n][d][w]: (E, t, D, B, A, rows)
    -- the estimate over the range, the best split (the largest D, the latest
    among equal ones; t = 0 and D = int64's minimum without a split) and
    whether B and A came from different rows there, no row giving both."""
    n, d, w = x.shape
    cand = np.asarray(cand, dtype=np.uint64)
    v = x[:, np.arange(d)[:, None], columns(cand, d, w)].astype(np.int64)  # [n][d][K]
    S, P = v.sum(axis=0), np.cumsum(v, axis=0)
    K = len(cand)
    bt, bD = np.zeros(K, np.int64), np.full(K, I64_MIN)
    bB, bA, rows = np.zeros(K, np.int64), np.zeros(K, np.int64), np.zeros(K, bool)
    for t in range(1, n):
        p, a = P[t - 1], S - P[t - 1]
        B, A = p.min(axis=0), a.min(axis=0)
        D = A * t - B * (n - t)
        D = -D if fall else D
        up = D >= bD
        bt[up], bD[up], bB[up], bA[up] = t, D[up], B[up], A[up]
        rows[up] = ~((p == B) & (a == A)).any(axis=0)[up]
    return S.min(axis=0).astype(np.uint64), bt, bD, bB.astype(np.uint64), bA.astype(np.uint64), rows


def onset(windows, first, last, cand, k, min_count=1, min_score=1, fall=False):
    """What sa_window_error_onset must return over the oracle's `windows` for
    first..last with the candidates `cand` (distinct, non-zero)."""
    cand = np.asarray(cand, dtype=np.uint64)
    x = window_cells(windows, first, last)
    E, t, D, B, A, _ = splits(x, cand, fall)
    mc, ms = max(int(min_count), 1), max(int(min_score), 1)
    elig = E >= np.uint64(mc)
    keep = np.flatnonzero(elig & (D >= ms)) if ms < 2**63 else np.zeros(0, np.int64)
    order = keep[np.lexsort((cand[keep], -D[keep]))]
    top = order[:k]
    return SimpleNamespace(keys=cand[top], onset_window=(t[top] + first).astype(np.uint64), score=D[top],
                           errors_before=B[top], errors_after=A[top], n_resident=len(cand), n_eligible=int(elig.sum()),
                           n_matched=len(order), error_spans=int(x[:, 0, :].sum(dtype=np.uint64)))


def items(r):
    return [tuple(int(v) for v in row) for row in zip(r.keys, r.onset_window, r.score, r.errors_before, r.errors_after)]


def assert_onset_equal(r, want, what):
    """An ErrorOnsetResult against onset()'s reference: every list and counter, bit for bit."""
    assert r.keys.dtype == r.onset_window.dtype == r.errors_before.dtype == r.errors_after.dtype == np.uint64, what
    assert r.score.dtype == np.int64, what
    got = (r.n_resident, r.n_eligible, r.n_matched, r.error_spans)
    assert got == (want.n_resident, want.n_eligible, want.n_matched, want.error_spans), ("counters", what, got)
    assert np.array_equal(r.keys, want.keys), ("keys", what)
    assert np.array_equal(r.score, want.score), ("score", what)
    assert np.array_equal(r.onset_window, want.onset_window), ("onset_window", what)
    assert np.array_equal(r.errors_before, want.errors_before), ("errors_before", what)
    assert np.array_equal(r.errors_after, want.errors_after), ("errors_after", what)
