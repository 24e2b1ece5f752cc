"""Heavy hitters over the window ring (sa_window_top): the cases' workloads and
their oracle answers, shared by tests/test_window_top_host.py (what the inputs
can catch, on the oracle alone) and tests/test_gpu_window_top.py (the kernels).

Cases of range_util are taken as they are (full:<row>, moved:ring_512, group).
The cases of this file:

  ties_small   ROWS["wide10"] (a small table, count-min 1 x 2): 1,050 keys, every
               estimate one of the two cells -- two tie classes of the whole table
  ties_binned  ROWS["binned5"] (a binned table, count-min 2 x 64): 60,000 keys,
               2 spans in 1,000 ERROR, so the cells are small numbers and the
               estimates fall into classes of thousands; TIES_BINNED_K cuts
               inside one
  cells128k, cells256k, cells1m
               a small table with 4 x 4,096, 8 x 4,096 and 4 x 32,768 cells
               (the default 4 x 2,048 is 64 KiB: sizes on both sides of any
               bound on what a workgroup stages)
  slots4096, slots8192
               tables of 4,096 slots (never more matches than SA_TOP_MAX_K, the
               pairs one workgroup sorts: the select has no work) and of 8,192
               with more than 4,096 matches: the smallest table on which it has

The reference: the oracle's cells of the range's windows summed as u64
(range_util.reference / merged), the candidates the distinct non-zero key_hash
of the batches ingested, the estimate sketch.cms_query's, the order
sketch.heavy_hitters' (estimate descending, then key ascending).  top() is that
vectorised; tests/test_window_top_host.py holds it against heavy_hitters.
"""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import pyoracle
import range_util
from geometry_util import config_of, key_pool, make_batch, ring_start
from ring_util import in_ring
from series_util import columns
from spanagg import Config

TOP_MAX_K = 4096
M64 = np.uint64(2**64 - 1)
TIES_SMALL_KS = (1, 7, 64, 65, TOP_MAX_K)
TIES_BINNED_K = 3000
CELL_SIZES = dict(cells128k=(4, 4096), cells256k=(8, 4096), cells1m=(4, 32768))
_SLOTS = dict(bounds=(1, 10, 100), hll_p=10, n_services=2, n_windows=2)
# name -> (row for assert_geometry or None, config, keys, spans, share of ERROR spans)
OWN = dict(ties_small=("wide10", config_of("wide10"), 1050, 60_000, 0.3),
           ties_binned=("binned5", config_of("binned5"), 60_000, 300_007, 0.002),
           **{name: (None, Config(key_capacity=1000, n_services=2, hll_p=10, n_windows=2, cms_d=d, cms_w=w), 700, 60_000,
                     0.3) for name, (d, w) in CELL_SIZES.items()},
           slots4096=(None, Config(key_capacity=3000, **_SLOTS), 2800, 120_000, 0.3),
           slots8192=(None, Config(key_capacity=6000, **_SLOTS), 5600, 120_000, 0.3))


@functools.lru_cache(maxsize=2)
def case(name):
    """range_util.case's shape: cfg, steps [(ring base, batch)], base, ranges, row."""
    if name not in OWN:
        return range_util.case(name)
    row, cfg, nk, n, share = OWN[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    w0 = ring_start(cfg)
    batch = make_batch(rng, n, cfg, nk, error_share=share, w0=w0, distinct_traces=True)
    return SimpleNamespace(name=name, cfg=cfg, steps=[(w0, batch)], keys=key_pool(nk)[:0], base=w0,
                           ranges=[(w0, w0 + cfg.n_windows - 1)], row=row)


@functools.lru_cache(maxsize=2)
def reference(name):
    """range_util.reference: the oracle's (registers, cells) of every window of the final ring."""
    if name not in OWN:
        return range_util.reference(name)
    c = case(name)
    cfg = c.cfg
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for base, batch in c.steps:
        o.ingest(in_ring(batch, cfg, base))
    seen = set(o.window_ids())
    zero = (np.zeros((cfg.n_services, 1 << cfg.hll_p), np.uint8), np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    return {w: o.window(w) if w in seen else zero for w in range(c.base, c.base + cfg.n_windows)}


def cells(windows, first, last) -> np.ndarray:
    """[d][w] u64: the cells of windows first..last summed (range_util.merged's)."""
    return range_util.merged(windows, range(first, last + 1), ()).cms


def candidates(batches) -> np.ndarray:
    """The distinct non-zero series of the batches, ascending."""
    k = np.unique(np.concatenate([b.key_hash for b in batches]))
    return k[k != 0]


def estimates(cms, keys) -> np.ndarray:
    """[n] u64: sketch.cms_query(cms, key) of every key."""
    d, w = cms.shape
    keys = np.asarray(keys, dtype=np.uint64)
    if len(keys) == 0:
        return np.zeros(0, np.uint64)
    return cms[np.arange(d)[:, None], columns(keys, d, w)].min(axis=0).astype(np.uint64)


def ranked(cms, cand, min_count=1, reverse_ties=False):
    """(keys, estimates) of the candidates with an estimate >= max(min_count,
    1), by estimate descending then key ascending (reverse_ties: descending)."""
    cand = np.asarray(cand, dtype=np.uint64)
    est = estimates(cms, cand)
    keep = est >= max(int(min_count), 1)
    cand, est = cand[keep], est[keep]
    order = np.lexsort((M64 - cand if reverse_ties else cand, M64 - est))
    return cand[order], est[order]


def top(cms, cand, k, min_count=1):
    """What sa_window_top must return over the summed cells `cms` with the
    candidates `cand` (distinct, non-zero)."""
    keys, est = ranked(cms, cand, min_count)
    return SimpleNamespace(keys=keys[:k], errors=est[:k], n_resident=len(cand), n_matched=len(keys),
                           error_spans=int(cms[0].sum(dtype=np.uint64)))


def items(t):
    return [(int(k), int(e)) for k, e in zip(t.keys, t.errors)]


def tie_class(est, k):
    """(start, size) of the run of equal estimates around position k - 1 of a
    ranked estimate list."""
    v = est[k - 1]
    idx = np.flatnonzero(est == v)
    return int(idx[0]), len(idx)


def assert_top_equal(r, want, what):
    """A TopResult against top()'s reference: every list and counter, bit for bit."""
    assert r.keys.dtype == np.uint64 and r.errors.dtype == np.uint64, what
    assert np.array_equal(r.keys, want.keys), ("keys", what)
    assert np.array_equal(r.errors, want.errors), ("errors", what)
    assert (r.n_resident, r.n_matched, r.error_spans) == (want.n_resident, want.n_matched, want.error_spans), \
        ("counters", what, r.n_resident, r.n_matched, r.error_spans)
