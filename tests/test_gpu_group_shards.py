"""Engine groups on crafted shards, merges and a moving ring, against the CPU oracle.

tests/test_gpu_group.py feeds groups random streams; here every input is built
to break something (tests/group_util.py; tests/test_group_host.py proves the
inputs on the CPU).  Members share device 0 and merge through device copies
(SA_OPT_GROUP_COPY); "both transports" adds a group of one over RCCL.  Every
comparison is bit-exact but the float sums (parity_util.SUM_RTOL).

  shard rule   a merged result cannot show which member took a span, so each
               member's `spans` counter is held against the count of its shard,
               for trace ids of every family (group_util.shard_words), spread
               four ways, through the host split and the device partition, at
               2, 3, 7, 63 and 64 members
  partition    batch sizes around the 1,024-span chunk, the last odd span, the
               step of the workgroup range at 2,097,153 spans, the host
               splitter's thread counts; a shard that takes everything
  staging      six device batches on two caller streams with growing shards
               and no host synchronisation in between
  flush merge  1, 2, 32, 33 and 63 (SA_MAX_BOUNDS + 1) buckets and three rows
               of geometry_util.ROWS: series on one member only, a member that
               holds none, traces that change members, an empty interval
  full table   one member's table overflows: SA_EFULL once, whole series
               dropped and counted, the next interval clean -- explicit and
               exponential
  fold         sa_group_flush_exp on the case families of group_util
  ring         ring_util.run_walk driven by groups

Interval 1 of the flush merge, as read here: members 0 and 1 each hold a set
of their own and share a third; member 2 receives spans without a key and
holds no series.  Interval 2 moves every trace one member on (member 0 holds
none), interval 4 feeds member 2 alone.
"""
import dataclasses
import functools
import time

import numpy as np
import pytest

import group_util as gu
import pyoracle
from geometry_util import check_against_oracle, config_of, key_pool, ring_start
from ring_util import run_walk, walk
from spanagg import Config, Engine, Group, SpanAggError, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

pytestmark = pytest.mark.gpu

U64 = np.uint64
TRANSPORTS = [(3, OPT_GROUP_COPY), (1, OPT_GROUP_RCCL)]
TRANSPORT_IDS = ["copy3", "rccl1"]


def _cfg(base=None, **kw) -> Config:
    return Config(**dict(base or gu.SMALL, **kw))


def _group(n, cfg, option=OPT_GROUP_COPY) -> Group:
    g = Group([0] * n, dataclasses.replace(cfg, options=cfg.options | option))
    assert g.size == n and g.uses_rccl == (option == OPT_GROUP_RCCL)
    g.window_advance(ring_start(cfg))
    return g


def _device(batch):
    """The batch's columns on device 0 (copied before this returns)."""
    import torch
    cols = [torch.from_numpy(c.view(np.int64 if c.dtype == np.uint64 else np.int32)).to("cuda:0")
            for c in batch.columns()]
    torch.cuda.synchronize()
    return cols


def _streams(k=2):
    import torch
    return [torch.cuda.Stream("cuda:0") for _ in range(k)]


def _feed(g, batch, route, stream=None):
    if route == "host":
        g.ingest(batch)
        return None
    cols = _device(batch)
    g.ingest_device(*cols, stream=stream)
    return cols  # (alive until the group's next sync)


def _spans(g):
    g.sync()
    return [s["spans"] for s in gu.member_stats(g)]


def _shard_case(g, cfg, n, size, dist, route, rng, earlier):
    """One batch of `size` spans spread by `dist`: every member's spans counter
    moves by its shard's count, then the flush, every window and the stats
    against the oracle fed the whole batch."""
    w1 = gu.mixed_words(n, gu.targets(n, size, dist), rng)
    b = gu.batch_for(cfg, w1, rng)
    before = _spans(g)
    keep = _feed(g, b, route)
    after = _spans(g)
    del keep
    assert [a - c for a, c in zip(after, before)] == gu.shard_counts(w1, n), (n, size, dist, route)
    check_against_oracle(g, [b], cfg, ring_start(cfg), earlier=earlier)
    earlier.append(b)


# ---- a. the shard rule on both routes ------------------------------------------------------------------------------

@pytest.mark.parametrize("route", ["host", "device"])
@pytest.mark.parametrize("n", [2, 3, 7])
def test_shard_rule(n, route):
    cfg, rng, earlier = _cfg(), np.random.default_rng([n, 0xA]), []
    with _group(n, cfg) as g:
        for dist in gu.DISTS:
            _shard_case(g, cfg, n, 4099, dist, route, rng, earlier)


@pytest.mark.parametrize("n", [63, 64])
def test_shard_rule_many_members(n):
    """Both routes and every distribution in one group: creating it is most of the cost (printed)."""
    cfg, rng, earlier = _cfg(), np.random.default_rng([n, 0xA]), []
    t0 = time.perf_counter()
    with _group(n, cfg) as g:
        print(f"group of {n} created in {time.perf_counter() - t0:.2f} s")
        for route in ("host", "device"):
            for dist in gu.DISTS:
                _shard_case(g, cfg, n, 4099, dist, route, rng, earlier)


# ---- b. partition sizes --------------------------------------------------------------------------------------------

DEVICE_SIZES = (1, 2, 1023, 1024, 1025, 2049, 65_537, 2_097_152, 2_097_153)
HOST_SIZES = (65_535, 65_536, 65_537, 1_048_576)
SIZE_CASES = [("device", s) for s in DEVICE_SIZES] + [("host", s) for s in HOST_SIZES]


@pytest.mark.parametrize("dist", ["skew0", "round_robin"])
@pytest.mark.parametrize("route,size", SIZE_CASES, ids=[f"{r}-{s}" for r, s in SIZE_CASES])
def test_partition_sizes(route, size, dist):
    cfg, rng = _cfg(), np.random.default_rng([size, 0xB])
    with _group(3, cfg) as g:
        _shard_case(g, cfg, 3, size, dist, route, rng, [])


# ---- c. staging sets -----------------------------------------------------------------------------------------------

def test_staging_sets_on_two_streams():
    cfg, rng, n = _cfg(), np.random.default_rng(0xC), 4
    sizes = (3001, 50_001, 7, 200_003, 1, 100_001)
    dists = ("round_robin", "skew0", "two_only", "one_each", "skew0", "round_robin")
    w1s = [gu.mixed_words(n, gu.targets(n, s, d), rng) for s, d in zip(sizes, dists)]
    batches = [gu.batch_for(cfg, w1, rng) for w1 in w1s]
    with _group(n, cfg) as g:
        cols = [_device(b) for b in batches]
        streams = _streams()
        for i, c in enumerate(cols):  # no host synchronisation of ours between the calls
            g.ingest_device(*c, stream=streams[i % 2].cuda_stream)
        want = np.sum([gu.shard_counts(w1, n) for w1 in w1s], axis=0).tolist()
        assert _spans(g) == want
        check_against_oracle(g, batches, cfg, ring_start(cfg))


# ---- d. flush merge at the bucket-count edges ----------------------------------------------------------------------

def _nbk_cfg(nbk) -> Config:
    """nbk buckets on a small table: bounds 2^(i/2) / 8 ms, the last below 2^48 ns."""
    return _cfg(bounds=tuple(2.0 ** (i / 2) / 8 for i in range(nbk - 1)), n_windows=2)


MERGE_CFGS = {f"nbk{k}": _nbk_cfg(k) for k in (1, 2, 32, 33, _lib.SA_MAX_BOUNDS + 1)}
MERGE_CFGS.update({row: config_of(row) for row in ("wide10", "part_generic", "atomic_nbk63")})
assert list(MERGE_CFGS)[:5] == ["nbk1", "nbk2", "nbk32", "nbk33", "nbk63"]


def _merge_intervals(cfg, rng):
    """The four intervals' batches for three members (module docstring);
    trace ids by member, so a group of one takes them as well."""
    pool = key_pool(24)
    own0, own1, both = pool[:8], pool[8:16], pool[16:]
    m = 1500
    which = rng.integers(0, 4, m)  # own0, own1, both, no key
    key = np.where(which < 3, pool[8 * np.minimum(which, 2) + rng.integers(0, 8, m)], U64(0))
    t = np.select([which == 0, which == 1, which == 2], [0, 1, rng.integers(0, 2, m)], 2)
    mk = lambda tt, kk: gu.batch_for(cfg, gu.mixed_words(3, tt, rng), rng, keys=kk, zero_share=0, max_log2=50)
    i1, i2 = mk(t, key), mk((t + 1) % 3, key)
    i4 = mk(np.full(500, 2), pool[rng.integers(0, 24, 500)])
    held = lambda b, j: set(b.key_hash[(b.trace_w1 % U64(3) == j) & (b.key_hash != 0)].tolist())
    assert not held(i1, 2) and not held(i2, 0) and held(i1, 0) & set(own0.tolist()) and not held(i1, 1) & set(own0.tolist())
    assert held(i2, 1) >= set(own0.tolist()) and not held(i4, 0) | held(i4, 1)
    return [i1, i2, None, i4]


@pytest.mark.parametrize("n,option", TRANSPORTS, ids=TRANSPORT_IDS)
@pytest.mark.parametrize("name", list(MERGE_CFGS))
def test_flush_merge_at_bucket_edges(name, n, option):
    cfg, rng = MERGE_CFGS[name], np.random.default_rng(0xD)
    w0, earlier = ring_start(cfg), []
    with _group(n, cfg, option) as g, Engine(cfg) as e:
        e.window_advance(w0)
        for b in _merge_intervals(cfg, rng):
            if b is not None:
                g.ingest(b)
                e.ingest(b)
                if n == 3:
                    assert _spans(g) == np.sum([gu.shard_counts(x.trace_w1, 3) for x in earlier + [b]], axis=0).tolist()
            rg = check_against_oracle(g, [] if b is None else [b], cfg, w0, earlier=earlier)
            re_ = e.flush()
            for f in ("key_hash", "bucket_counts", "calls", "sum_ns", "sum"):  # one engine, column for column
                va, vb = getattr(rg, f), getattr(re_, f)
                assert va.shape == vb.shape and va.tobytes() == vb.tobytes(), (name, f)
            assert (b is None) == (len(rg.key_hash) == 0)
            if b is not None:
                earlier.append(b)
                if name.startswith("nbk") and cfg.bounds:  # the first and the last bucket hold spans
                    assert rg.bucket_counts[:, -1].sum() > 0 and rg.bucket_counts[:, 0].sum() > 0, name


# ---- e. a full table on one member -----------------------------------------------------------------------------------

def _full_batches(cfg, rng):
    """Interval 1: 40 series on member 0 and 4 each on members 1 and 2 (16
    slots a member); interval 2: 4 series a member."""
    pool = key_pool(48)
    sets = [pool[:40], pool[40:44], pool[44:48]]
    out = []
    for per in ((40, 4, 4), (4, 4, 4)):
        t = np.concatenate([np.full(600, 0), np.full(60, 1), np.full(60, 2)])
        key = np.concatenate([np.resize(sets[j][:per[j]], int((t == j).sum())) for j in range(3)])
        out.append(gu.batch_for(cfg, gu.mixed_words(3, t, rng), rng, keys=key, zero_share=0.02))
    return out


def _rows_of(res, cfg):
    """key -> the row's comparable content."""
    if cfg.exp_max_size:
        return {int(k): (int(res.count[i]), int(res.zero_count[i]), int(res.scale[i]), int(res.offset[i]),
                         [int(x) for x in res.buckets[i]]) for i, k in enumerate(res.key_hash)}
    return {int(k): (int(res.calls[i]), int(res.sum_ns[i]), res.bucket_counts[i].tolist())
            for i, k in enumerate(res.key_hash)}


def _oracle_rows(b, cfg):
    if cfg.exp_max_size:
        ora = pyoracle.expo_aggregate(b, cfg.exp_max_size, cfg.unit == "s")
        return {k: (o["count"], o["zero_count"], o["scale"], o["offset"], [int(x) for x in o["counts"]])
                for k, o in ora.items()}
    o = _oracle(cfg, [b]).series()
    return {int(k): (int(o["calls"][i]), int(o["sum_ns"][i]), o["bucket_counts"][i].tolist())
            for i, k in enumerate(o["key_hash"])}


def _oracle(cfg, batches):
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for b in batches:
        o.ingest(b)
    return o


def _assert_windows(g, cfg, batches):
    o = _oracle(cfg, batches)
    seen, w0 = set(o.window_ids()), ring_start(cfg)
    for wid in range(w0, w0 + cfg.n_windows):
        sk = g.window_read(wid)
        assert wid in seen
        hll, cms = o.window(wid)
        assert np.array_equal(sk.hll, hll) and np.array_equal(sk.cms, cms), wid


@pytest.mark.parametrize("expo", [False, True], ids=["explicit", "expo"])
def test_full_table_on_one_member(expo):
    cfg = _cfg(key_capacity=8, **({"exp_max_size": 12} if expo else {}))
    first, second = _full_batches(cfg, np.random.default_rng(0xE))
    flush = lambda g, **kw: g.flush_exp(**kw) if expo else g.flush(**kw)
    count = lambda r: int((r.count if expo else r.calls).sum())
    with _group(3, cfg) as g:  # without allow_drops: the error
        g.ingest(first)
        with pytest.raises(SpanAggError) as x:
            flush(g)
        assert x.value.code == _lib.SA_EFULL
    with _group(3, cfg) as g:
        assert [s["table_capacity"] for s in gu.member_stats(g)] == [16, 16, 16]
        g.ingest(first)
        res = flush(g, allow_drops=True)
        assert res.status == _lib.SA_EFULL
        st = g.stats()
        zero = int((first.key_hash == 0).sum())
        assert st["zero_key"] == zero and st["spans"] == len(first)
        assert count(res) + st["dropped_table_full"] == len(first) - zero
        drops = [s["dropped_table_full"] for s in gu.member_stats(g)]
        assert drops[0] > 0 and drops[1:] == [0, 0]
        got, ora = _rows_of(res, cfg), _oracle_rows(first, cfg)
        assert len(got) == 16 + 8 and all(ora[k] == row for k, row in got.items())  # whole series, 24 of member 0's dropped
        assert st["dropped_table_full"] == sum(ora[k][0] for k in set(ora) - set(got))
        _assert_windows(g, cfg, [first])  # the sketches hold every span
        # the next interval, few series: no error, drops counted once
        g.ingest(second)
        res = flush(g)
        assert res.status == 0 and _rows_of(res, cfg) == _oracle_rows(second, cfg)
        assert g.stats()["dropped_table_full"] == st["dropped_table_full"]
        _assert_windows(g, cfg, [first, second])
        assert len(flush(g).key_hash) == 0


# ---- f. the fold on the device ---------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _fold_intervals(n, unit):
    """Two intervals of 64 series, eight of every family of group_util.FAMILIES,
    at most 40 spans each, every span on the member its family says."""
    cfg, rng = _cfg(unit=unit), np.random.default_rng([n, 0xF, unit == "s"])
    pool, out = key_pool(64), []
    for _ in range(2):
        key, dur, t = [], [], []
        for j, k in enumerate(pool):
            family = gu.FAMILIES[j % len(gu.FAMILIES)]
            m = 20 if family == "near_1ms" else int(rng.integers(2, 41))
            d = gu.series_durations(family, rng, m)
            t.append(gu.series_shards(family, rng, m, n, d))
            dur.append(d)
            key.append(np.full(m, k, dtype=U64))
        key, dur, t = (np.concatenate(x) for x in (key, dur, t))
        order = rng.permutation(len(key))
        out.append(gu.batch_for(cfg, gu.mixed_words(n, t[order], rng), rng, keys=key[order], zero_share=0, dur=dur[order]))
    return tuple(out)


@pytest.mark.parametrize("unit", ["ms", "s"])
@pytest.mark.parametrize("max_size", [2, 3, 160, 4096])
@pytest.mark.parametrize("n", [2, 3, 5])
def test_fold_on_the_device(n, max_size, unit):
    cfg = _cfg(unit=unit, exp_max_size=max_size)
    earlier = []
    with _group(n, cfg) as g:
        for b in _fold_intervals(n, unit):
            g.ingest(b)
            assert _spans(g) == np.sum([gu.shard_counts(x.trace_w1, n) for x in earlier + [b]], axis=0).tolist()
            check_against_oracle(g, [b], cfg, ring_start(cfg), earlier=earlier)  # (parity_util._check: the fold)
            earlier.append(b)


# ---- g. the moving ring ------------------------------------------------------------------------------------------------

class GroupDeviceFeed:
    """ring_util.DeviceFeed for a group: the walk's batches on device 0, copied
    once; consecutive Group.ingest_device calls alternate between two streams
    that waited for the copies, with no host synchronisation afterwards."""

    def __init__(self, g, wk):
        import torch
        self.g, self.launches = g, 0
        self.cols = {name: _device(b) for name, b in wk.batches.items()}
        self.streams = _streams()
        for s in self.streams:
            s.wait_stream(torch.cuda.current_stream("cuda:0"))

    def __call__(self, name):
        s = self.streams[self.launches % 2].cuda_stream
        self.launches += 1
        self.g.ingest_device(*self.cols[name], stream=s)


RING_CASES = [("ring_512", 3, OPT_GROUP_COPY), ("ring_default", 1, OPT_GROUP_RCCL),
              ("ring_expo_generic", 2, OPT_GROUP_COPY), ("ring_part", 2, OPT_GROUP_COPY)]


@pytest.mark.parametrize("mode", ["host", "device"])
@pytest.mark.parametrize("row,n,option", RING_CASES, ids=[c[0] for c in RING_CASES])
def test_ring_walk_by_a_group(row, n, option, mode):
    wk = walk(row)
    cfg = config_of(row)
    with Group([0] * n, dataclasses.replace(cfg, options=cfg.options | option)) as g:
        assert g.size == n and g.uses_rccl == (option == OPT_GROUP_RCCL)
        feed = (lambda name: g.ingest(wk.batches[name])) if mode == "host" else GroupDeviceFeed(g, wk)
        run_walk(g, row, feed)
