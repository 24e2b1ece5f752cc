"""GPU parity of dense-index engines (SA_OPT_DENSE_IDS, spanagg_dense.hip:
bt_scatter2_kernel<BtDense> + dn_aggregate_kernel, sa_bind_ids) against the
CPU oracle fed the real series hashes.  The scatter's launch-size and
record-limit edges run on a default (hashed) engine of the same table too: one
kernel template serves both.

Bar: parity_util.assert_red_equal (bucket counts, calls and ns sums bit-exact,
sums within 1e-9 relative); HLL registers and count-min cells np.array_equal
for every oracle window.  key_capacity=300_000 gives 2^19 table slots, 256 per
bin, unless stated.
"""
import functools

import numpy as np
import pytest

import pyoracle
from parity_util import assert_red_equal
from spanagg import Config, Engine, Group, SpanAggError, SpanBatch, bucket_thresholds, pack_meta
from spanagg import _lib
from spanagg._lib import OPT_DENSE_IDS
from spanagg.synth import generate_highcard

pytestmark = pytest.mark.gpu

CAP = 1 << 19  # table_capacity at key_capacity=300_000


def _oracle(*batches):
    o = pyoracle.Oracle(n_services=1)
    for b in batches:
        o.ingest(b)
    return o


def _engine(options, kcap=300_000, n_windows=16):
    e = Engine(Config(n_services=1, n_windows=n_windows, key_capacity=kcap, options=options))
    st = e.stats()
    assert st["small_table"] == 0 and st["n_keys"] == 0
    return e


def _dense(kcap=300_000, n_windows=16):
    return _engine(OPT_DENSE_IDS, kcap, n_windows)


BOTH = pytest.mark.parametrize("options", [0, OPT_DENSE_IDS], ids=["hashed", "dense"])


def _with_keys(batch, keys):
    return SpanBatch(keys, *batch.columns()[1:])


def _take(batch, sel):
    return SpanBatch(*[c[sel] for c in batch.columns()])


def _dev(arrays):
    import torch
    dev = torch.device("cuda", 0)
    out = [torch.from_numpy(np.ascontiguousarray(c).view(np.int64 if c.dtype == np.uint64 else np.int32)).to(dev)
           for c in arrays]
    torch.cuda.synchronize(dev)
    return out


def _check_windows(e, o_hll, o_cms=None):
    """HLL of every window of o_hll, count-min of the same windows of o_cms."""
    o_cms = o_cms or o_hll
    assert o_hll.window_ids()
    for wid in o_hll.window_ids():
        sk = e.window_read(wid)
        hll, _ = o_hll.window(wid)
        assert np.array_equal(sk.hll, hll), wid
        cms = o_cms.window(wid)[1] if wid in o_cms.window_ids() else np.zeros_like(sk.cms)
        assert np.array_equal(sk.cms, cms), wid


def _check(e, o, n_spans):
    res = e.flush()
    assert_red_equal(res, o.series())
    _check_windows(e, o)
    st = e.stats()
    assert st["dropped_table_full"] == 0
    assert int(res.calls.sum()) == n_spans - st["zero_key"]
    return res


@functools.lru_cache(maxsize=None)
def _workload(zipf):
    batch, _, w0 = generate_highcard(2_000_000, seed=61, routes=500, pods=300, zipf_s=zipf)
    return batch, w0, _oracle(batch)


@pytest.mark.parametrize("zipf", [0.0, 1.3], ids=["uniform", "zipf1.3"])
def test_host_batches_match_oracle_and_default_engine(zipf):
    """2 M spans over 150 k series through Engine.ingest in two halves (real
    hashes: the engine encodes and binds), on a dense and on a default engine.
    The Zipf mix runs the overflow table and region overflow."""
    batch, w0, o = _workload(zipf)
    half = len(batch) // 2
    for opt in (OPT_DENSE_IDS, 0):
        with Engine(Config(n_services=1, n_windows=16, key_capacity=300_000, options=opt)) as e:
            e.window_advance(w0)
            e.ingest(batch.slice(0, half))
            e.ingest(batch.slice(half, len(batch)))
            res = _check(e, o, len(batch))
            if opt:
                assert e.stats()["n_keys"] == len(res.key_hash) == len(e.ids)


def test_one_hot_series_twice_before_flush():
    """1.5 M spans in one launch, 70 % on one series, 20 % on 200 warm series
    (1,500 spans each: u8 row counts pass 255 in the aggregate's write-back),
    the rest uniform; the same batch again before the flush.  The hot series
    lives in every scatter workgroup's overflow table (u16 counts, bounded by
    the spans a workgroup takes per launch)."""
    n = 1_500_000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(67))
    u = rng.random(n)
    keys = base.key_hash.copy()
    keys[u < 0.7] = np.uint64(0xC0FFEE0DDBA11)
    warm = rng.integers(1, 2**63, 200, dtype=np.int64).astype(np.uint64)
    sel = (u >= 0.7) & (u < 0.9)
    keys[sel] = warm[rng.integers(0, 200, int(sel.sum()))]
    batch = _with_keys(base, keys)
    o = _oracle(batch, batch)
    with _dense() as e:
        e.window_advance(w0)
        ids, ni, nh = e.ids.encode(batch.key_hash)
        e.bind_ids(ni, nh)
        cols = _dev((ids,) + batch.columns()[1:])
        e.ingest_device(*cols, n=n)
        e.ingest_device(*cols, n=n)
        res = _check(e, o, 2 * n)
        assert int(res.calls.max()) > 2 * 0.69 * n


@functools.lru_cache(maxsize=None)
def _edge_batch():
    thr, _ = bucket_thresholds(Config().bounds)
    edges = ([0] + [int(t) + k for t in thr for k in (-1, 0, 1)] +
             [2**37 - 1, 2**37, 2**42, 2**59 - 1, 2**59])
    n = 4000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(71))
    d = np.array(edges, dtype=np.uint64)[rng.integers(0, len(edges), n)]
    d[: len(edges)] = np.array(edges, dtype=np.uint64)  # every edge at least once
    kidx = rng.integers(0, 50, n)
    kidx[n - 3:] = [7, 21, 42]
    d[n - 3:] = np.uint64(2**63)
    end = base.start_ns.copy()  # the generator's start times as end times: inside the window ring ...
    start = end - d             # ... and every span starts d earlier
    start[1] = end[1] + np.uint64(12345)  # end < start
    long = d == np.uint64(2**63)
    start[long] = base.start_ns[long]
    end[long] = base.start_ns[long] + np.uint64(2**63)  # (these end far outside the window ring)
    keys = rng.integers(1, 2**63, 50, dtype=np.int64).astype(np.uint64)[kidx]
    status = np.where(rng.random(n) < 0.3, 2, 0)
    status[n - 2] = 2
    batch = SpanBatch(keys, start, end, base.trace_w0, base.trace_w1, pack_meta(np.zeros(n, np.uint32), 2, status))
    o = _oracle(batch)
    ref = o.series()
    assert np.allclose(ref["sum_ns"].astype(np.float64) / 1e6, ref["sum_go"], rtol=1e-9)  # (no u64 sum wrapped)
    return batch, w0, o, long


@BOTH
def test_duration_edges(options):
    """Durations 0, end < start, each default threshold and +-1 ns, and the
    records' limits: 2^37 - 1 stays in a dense record, 2^37 and longer take
    its cold path; 2^59 - 1 stays in a hashed record, 2^59 takes its cold
    path; also 2^42 and 2^63 ns.  ERROR spans among them, over 50 series.  A
    series' ns sum is a u64 everywhere (engine, oracle, result): the 2^63-ns
    spans go to three series, one each, so no sum wraps."""
    batch, w0, o, long = _edge_batch()
    n = len(batch)
    with _engine(options) as e:
        e.window_advance(w0)
        e.ingest(batch)
        res = e.flush()
        assert_red_equal(res, o.series())
        assert int(res.calls.sum()) == n
        st = e.stats()
        assert st["dropped_table_full"] == 0 and st["window_out_of_range"] == int(long.sum()) > 0
        # the oracle keeps windows outside the ring too; the resident ones must match
        wids = [w for w in o.window_ids() if w0 <= w < w0 + 16]
        assert wids
        for wid in wids:
            sk = e.window_read(wid)
            hll, cms = o.window(wid)
            assert np.array_equal(sk.hll, hll) and np.array_equal(sk.cms, cms), wid


@BOTH
@pytest.mark.parametrize("n", [1, 127, 4097, 8193])
def test_ragged_launch_sizes(n, options):
    """One and two scatter workgroups, partial tiles and partial stages."""
    base, w0, _ = _workload(0.0)
    batch = base.slice(1000, 1000 + n)
    with _engine(options) as e:
        e.window_advance(w0)
        keys = batch.key_hash
        if options & OPT_DENSE_IDS:
            keys, ni, nh = e.ids.encode(batch.key_hash)
            e.bind_ids(ni, nh)
        e.ingest_device(*_dev((keys,) + batch.columns()[1:]), n=n)
        _check(e, _oracle(batch), n)


def test_index_geometry_device_path():
    """Hand-made indices through ingest_device and bind_ids: the first and
    last index, indices around a bin wrap, a set that shares one bin and a set
    that shares one in-bin slot across bins; index 0 counts in zero_key;
    table_capacity and 2^64 - 1 count in dropped_table_full (flush: SA_EFULL),
    raise their HLL registers and touch no count-min cell."""
    n = 200_000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(73))
    valid = np.unique(np.array([1, 2047, 2048, 2049, CAP - 1] +
                               [5 + 2048 * s for s in range(0, 256, 5)] +      # bin 5, in-bin slots 0, 5, ..
                               [3 * 2048 + b for b in range(0, 2048, 37)],     # in-bin slot 3 of many bins
                               dtype=np.uint64))
    hashes = rng.integers(1, 2**63, len(valid), dtype=np.int64).astype(np.uint64)
    assert len(np.unique(hashes)) == len(valid)
    pick = rng.integers(0, len(valid), n)
    idx = valid[pick]
    keys = hashes[pick]
    u = rng.random(n)
    zero, big1, big2 = u < 0.01, (u >= 0.01) & (u < 0.02), (u >= 0.02) & (u < 0.03)
    idx[zero] = 0
    idx[big1] = CAP
    idx[big2] = 2**64 - 1
    ok = ~(zero | big1 | big2)
    # (index-0 spans carry no ERROR status: what they add to the count-min is
    # the default engine's business, not this option's)
    meta = base.meta.copy()
    meta[zero] = pack_meta(0, 2, 0)
    batch = SpanBatch(keys, base.start_ns, base.end_ns, base.trace_w0, base.trace_w1, meta)
    o_valid = _oracle(_take(batch, ok))
    o_all = _oracle(batch)
    with _dense() as e:
        assert e.stats()["table_capacity"] == CAP
        e.window_advance(w0)
        e.bind_ids(valid, hashes)
        assert e.stats()["n_keys"] == len(valid)
        e.ingest_device(*_dev((idx,) + batch.columns()[1:]), n=n)
        with pytest.raises(SpanAggError) as x:
            e.flush()
        assert x.value.code == _lib.SA_EFULL
        st = e.stats()
        assert st["zero_key"] == int(zero.sum()) > 0
        assert st["dropped_table_full"] == int(big1.sum() + big2.sum()) > 0
        # the same spans again: the flush above reset the delta and reported the drops
        e.ingest_device(*_dev((idx,) + batch.columns()[1:]), n=n)
        res = e.flush(allow_drops=True)
        assert res.status == _lib.SA_EFULL
        assert_red_equal(res, o_valid.series())
        _check_windows(e, o_all, _oracle(_take(batch, ok), _take(batch, ok)))


def test_unbound_index_is_dropped_at_flush():
    """Spans on a valid index that was never bound: counted dropped by the time
    flush returns (SA_EFULL), no row, no count-min cell; the others exact."""
    n = 50_000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(79))
    idx = rng.integers(1, 111, n).astype(np.uint64)  # 1..100 bound, 101..110 never
    hashes = rng.integers(1, 2**63, 111, dtype=np.int64).astype(np.uint64)
    status = np.where(rng.random(n) < 0.2, 2, 0)
    batch = SpanBatch(hashes[idx.astype(np.int64)], base.start_ns, base.end_ns, base.trace_w0, base.trace_w1,
                      pack_meta(np.zeros(n, np.uint32), 2, status))
    bound = idx <= 100
    o_bound = _oracle(_take(batch, bound))
    with _dense() as e:
        e.window_advance(w0)
        e.bind_ids(np.arange(1, 101, dtype=np.uint64), hashes[1:101])
        e.ingest_device(*_dev((idx,) + batch.columns()[1:]), n=n)
        res = e.flush(allow_drops=True)
        assert res.status == _lib.SA_EFULL
        assert e.stats()["dropped_table_full"] == int((~bound).sum()) > 0
        assert_red_equal(res, o_bound.series())
        assert not np.isin(hashes[101:], res.key_hash).any()
        _check_windows(e, _oracle(batch), o_bound)
        # binding one of them afterwards starts it from nothing
        e.bind_ids([101], [hashes[101]])
        res = e.flush()
        assert len(res.key_hash) == 0
        _check_windows(e, _oracle(batch), o_bound)


def test_pipeline_new_series_every_launch():
    """Six device launches of 300 k spans alternating over two streams, new
    series bound before each; one flush.  Then a second interval through
    ingest_device_many (k = 3): the delta restarts, the sketches go on."""
    import torch
    dev = torch.device("cuda", 0)
    n = 300_000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(83))
    streams = [torch.cuda.Stream(dev) for _ in range(2)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream(dev))
    rest = _dev(base.columns()[1:])
    with _dense(1_200_000, n_windows=16) as e:
        e.window_advance(w0)
        batches, key_cols = [], []
        for i in range(6):
            c = np.uint64(rng.integers(1, 2**63 - 1))
            b = _with_keys(base, base.key_hash ^ c)
            ids, ni, nh = e.ids.encode(b.key_hash)
            assert len(ni) > 0
            e.bind_ids(ni, nh)
            (k,) = _dev((ids,))
            key_cols.append(k)
            batches.append(b)
            e.ingest_device(k, *rest, n=n, stream=streams[i % 2].cuda_stream)
        torch.cuda.synchronize(dev)
        o = _oracle(*batches)
        res = _check(e, o, 6 * n)
        assert len(np.unique(res.key_hash)) == len(res.key_hash) == e.stats()["n_keys"]
        e.ingest_device_many([(key_cols[i], *rest, n) for i in range(3)], stream=streams[0].cuda_stream)
        torch.cuda.synchronize(dev)
        res = e.flush()
        assert_red_equal(res, _oracle(*batches[:3]).series())
        _check_windows(e, _oracle(*batches, *batches[:3]))
        assert e.stats()["dropped_table_full"] == 0


def test_recycling_an_index():
    """bind_ids on a bound index: SA_ESTATE with unflushed spans, fine after a
    flush; the old series' ERROR spans stay in the old hash's count-min cells
    and the new series' spans come back under the new hash."""
    n = 20_000
    base, w0, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(89))
    idx = rng.integers(1, 21, n).astype(np.uint64)
    old = rng.integers(1, 2**63, 21, dtype=np.int64).astype(np.uint64)
    new = old.copy()
    new[5] = np.uint64(0xABCDEF0123456789)
    new[6] = np.uint64(0x1234567)
    status = np.where(rng.random(n) < 0.3, 2, 0)
    cols = (base.start_ns, base.end_ns, base.trace_w0, base.trace_w1, pack_meta(np.zeros(n, np.uint32), 2, status))
    b_old = SpanBatch(old[idx.astype(np.int64)], *cols)
    b_new = SpanBatch(new[idx.astype(np.int64)], *cols)
    with _dense() as e:
        e.window_advance(w0)
        e.bind_ids(np.arange(1, 21, dtype=np.uint64), old[1:])
        dcols = _dev((idx,) + cols)
        e.ingest_device(*dcols, n=n)
        with pytest.raises(SpanAggError) as x:
            e.bind_ids([5, 6], [new[5], new[6]])
        assert x.value.code == _lib.SA_ESTATE
        assert_red_equal(e.flush(), _oracle(b_old).series())
        e.bind_ids([5, 6], [new[5], new[6]])  # no window was read in between: the bind folds the ERROR counts
        assert e.stats()["n_keys"] == 20
        e.ingest_device(*dcols, n=n)
        res = e.flush()
        assert_red_equal(res, _oracle(b_new).series())
        assert np.isin(new[5:7], res.key_hash).all() and not np.isin(old[5:7], res.key_hash).any()
        _check_windows(e, _oracle(b_old, b_new))
        assert e.stats()["dropped_table_full"] == 0


def test_wide_table():
    """2^22 slots (2,048 per bin: the aggregate's largest LDS form), 8
    windows; 1 M uniform spans over 2 M series."""
    n = 1_000_000
    base, _, _ = _workload(0.0)
    base = base.slice(0, n)
    rng = np.random.Generator(np.random.PCG64(97))
    pool = rng.integers(1, 2**63, 2_000_000, dtype=np.int64).astype(np.uint64)
    t0 = base.start_ns.min() // np.uint64(10**10) * np.uint64(10**10)
    start = t0 + (base.start_ns - t0) // np.uint64(6)  # starts over 10 s instead of 60
    end = start + (base.end_ns - base.start_ns)       # <= 60 s long: at most 7 windows of 10 s
    batch = SpanBatch(pool[rng.integers(0, len(pool), n)], start, end, base.trace_w0, base.trace_w1, base.meta)
    w0 = int(end.min()) // 10**10
    o = _oracle(batch)
    assert max(o.window_ids()) < w0 + 8
    with _dense(3_000_000, n_windows=8) as e:
        assert e.stats()["table_capacity"] == 1 << 22
        e.window_advance(w0)
        e.ingest(batch)
        res = _check(e, o, n)
        assert len(res.key_hash) > 700_000


def test_hooks_on_a_dense_engine():
    import torch
    dev = torch.device("cuda", 0)
    n = 30_000
    base, w0, _ = _workload(0.0)
    batch = base.slice(0, n)
    with _dense() as e:
        e.window_advance(w0)
        e.ingest(batch)
        extra = np.array([0x1111, 0x2222], dtype=np.uint64)  # bound, no spans: no delta
        _, ni, nh = e.ids.encode(extra)
        e.bind_ids(ni, nh)
        uniq = np.unique(batch.key_hash)
        assert e.stats()["n_keys"] == len(uniq) + 2
        d_keys = torch.zeros(len(uniq) + 16, dtype=torch.int64, device=dev)
        got = e.export_keys(d_keys, len(uniq) + 16)
        assert got == len(uniq)
        assert np.array_equal(np.sort(d_keys[:got].cpu().numpy().view(np.uint64)), uniq)
        d_rows = torch.zeros((got, e.n_buckets + 1), dtype=torch.int64, device=dev)
        for call in (lambda: e.gather_dense(d_keys, got, d_rows, False), lambda: e.reclaim_keys(True),
                     lambda: e.reclaim_keys(False)):
            with pytest.raises(SpanAggError) as x:
                call()
            assert x.value.code == _lib.SA_ESTATE
        assert_red_equal(e.flush(), _oracle(batch).series())
    with pytest.raises(SpanAggError) as x:
        Group([0], Config(n_services=1, key_capacity=300_000, options=OPT_DENSE_IDS))
    assert x.value.code == _lib.SA_EINVAL
    with Engine(Config(n_services=1, key_capacity=300_000)) as e:  # bind_ids needs the option
        with pytest.raises(SpanAggError) as x:
            e.bind_ids([1], [5])
        assert x.value.code == _lib.SA_ESTATE
    with _dense() as e:  # sa_bind_ids' argument checks
        for i, h in ((0, 5), (CAP, 5), (2**64 - 1, 5), (7, 0)):
            with pytest.raises(SpanAggError) as x:
                e.bind_ids([i], [h])
            assert x.value.code == _lib.SA_EINVAL
        assert e.stats()["n_keys"] == 0
