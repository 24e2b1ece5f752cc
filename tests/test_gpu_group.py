"""Engine groups (include/spanagg.h sa_group_*): several engines behind one
handle, spans sharded by trace id, merged at flush / window read.  On the
one-GPU lease both transports run: two members on device 0 merge through
device copies + a reduce kernel, a group of one with SA_OPT_GROUP_RCCL
merges over a one-rank RCCL communicator.  Bar: the merge equals the CPU
oracle fed the whole stream (bucket counts, calls, ns sums, HLL registers and
count-min cells bit-exact; duration sums within 1e-9 relative)."""
import dataclasses
import functools

import numpy as np
import pytest

import pyoracle
from geometry_util import key_pool, make_batch, ring_start
from parity_util import assert_red_equal
from spanagg import _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL, OPT_WINDOW_LATENCY
from spanagg import Config, Engine, Group, SpanAggError, SpanBatch
from spanagg.synth import generate_c2, generate_highcard

pytestmark = pytest.mark.gpu


def _check_windows(g, o):
    for wid in o.window_ids():
        sk = g.window_read(wid)
        hll, cms = o.window(wid)
        assert np.array_equal(sk.hll, hll), wid
        assert np.array_equal(sk.cms, cms), wid


@pytest.mark.parametrize("devices,rccl", [([0, 0], False), ([0, 0, 0], False), ([0], True)])
def test_group_matches_oracle_c2(devices, rccl):
    wl = generate_c2(400_003, seed=21)
    opt = OPT_GROUP_RCCL if rccl else OPT_GROUP_COPY
    with Group(devices, Config(n_services=wl.n_services, n_windows=16, options=opt)) as g:
        assert g.size == len(devices)
        assert g.uses_rccl == rccl
        g.window_advance(wl.first_window)
        g.ingest(wl.batch)
        res = g.flush()
        o = pyoracle.Oracle(n_services=wl.n_services)
        o.ingest(wl.batch)
        assert_red_equal(res, o.series())
        _check_windows(g, o)
        st = g.stats()
        assert st["spans"] == len(wl.batch)
        # members keep their keys, or the flush emptied their more than half
        # full tables (sa_reclaim_keys; 2,048 slots each here)
        assert st["n_keys"] == 0 or st["n_keys"] >= len(res.key_hash)


def test_group_delta_flushes_and_equals_one_engine():
    wl = generate_c2(300_000, seed=5)
    a, b = wl.batch.slice(0, 170_000), wl.batch.slice(170_000, 300_000)
    cfg = Config(n_services=wl.n_services, n_windows=16, options=OPT_GROUP_COPY)
    with Group([0, 0], cfg) as g, Engine(cfg) as e:
        for x in (g, e):
            x.window_advance(wl.first_window)
        for part in (a, b):
            g.ingest(part)
            e.ingest(part)
            rg, re_ = g.flush(), e.flush()
            assert np.array_equal(rg.key_hash, re_.key_hash)
            assert np.array_equal(rg.bucket_counts, re_.bucket_counts)
            assert np.array_equal(rg.sum_ns, re_.sum_ns)
        empty = g.flush()  # nothing since the last flush
        assert len(empty.key_hash) == 0


def test_group_high_cardinality_binned_members():
    """Members on the binned HBM-table path (1 M keys): the key union spans
    series seen by one member only and by both."""
    batch, _, first = generate_highcard(1_500_000, seed=3)
    with Group([0, 0], Config(n_services=1, n_windows=16, key_capacity=1_200_000, options=OPT_GROUP_COPY)) as g:
        g.window_advance(first)
        g.ingest(batch)
        res = g.flush()
        o = pyoracle.Oracle(n_services=1)
        o.ingest(batch)
        assert_red_equal(res, o.series())
        _check_windows(g, o)


def test_group_rejects_bad_arguments():
    with pytest.raises(Exception):
        Group([], Config())


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_group_exponential_histograms_fold_to_one_engine(devices):
    """sa_group_flush_exp: each member's delta exponential histograms (its own
    trace-id shard, so its own scales) folded per series on the host must be
    the histogram of the whole stream, bit-exact against the go-expohisto
    restatement, over two flush intervals."""
    wl = generate_c2(300_000, seed=31)
    parts = [wl.batch.slice(0, 120_000), wl.batch.slice(120_000, 300_000)]
    with Group(devices, Config(n_services=wl.n_services, n_windows=16, exp_max_size=12)) as g:
        g.window_advance(wl.first_window)
        for part in parts:
            g.ingest(part)
            res = g.flush_exp()
            ora = pyoracle.expo_aggregate(part, 12)
            assert [int(k) for k in res.key_hash] == sorted(ora)
            for i, k in enumerate(res.key_hash):
                o = ora[int(k)]
                assert (int(res.count[i]), int(res.zero_count[i]), int(res.scale[i]), int(res.offset[i])) == \
                    (o["count"], o["zero_count"], o["scale"], o["offset"]), k
                assert [int(x) for x in res.buckets[i]] == [int(x) for x in o["counts"]], k
                assert res.min[i] == o["min"] and res.max[i] == o["max"]
        with pytest.raises(Exception):
            g.flush()  # explicit-bucket flush of an exponential group: SA_ESTATE
        o = pyoracle.Oracle(n_services=wl.n_services)
        o.ingest(wl.batch)
        _check_windows(g, o)


# ---- the window queries: one merge path and one ending for all of them -------
# Two members on device 0 merge through device copies; a group of one that asks
# for RCCL all-reduces for real.  (The queries' own files, test_gpu_window_*.py,
# hold each query's group case against the oracle on larger rings; here every
# group query runs on both transports against one engine, and after a failure.)
QCFG = Config(n_services=3, n_windows=4, key_capacity=1500, options=OPT_WINDOW_LATENCY)
TRANSPORTS = [([0, 0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True)]
SUMMED = ("n_resident", "n_matched")  # of top and movers: a group's are its members' sums


@functools.lru_cache(maxsize=1)
def _query_case():
    """The ring's first window and 2,000 spans over its four windows, ~30 % of them ERROR."""
    return ring_start(QCFG), make_batch(np.random.default_rng(0x9A7E), 2000, QCFG, 300)


def _queries(base, last=None, k=10):
    """name -> the call on an Engine or a Group; `last` and `k` as the failing calls bend them."""
    first, last = base, base + 3 if last is None else last
    keys = key_pool(300)[:16]
    return {
        "window_read": lambda x: x.window_read(first + 1),
        "window_range": lambda x: x.window_range(first, last, keys, registers=True, cells=True),
        "window_top": lambda x: x.window_top(first, last, k),
        "window_movers": lambda x: x.window_movers((first, first + 1), (first + 2, last), k),
        "window_overlap": lambda x: x.window_overlap(first, last),
        "window_latency": lambda x: x.window_latency_series(first + 1, last, 2, hist=True),
        "window_latency_movers": lambda x: x.window_latency_movers((first, first + 1), (first + 2, last), min(k, 3)),
    }


def _loaded(cls, *args):
    base, batch = _query_case()
    x = cls(*args)
    x.window_advance(base)
    x.ingest(batch)
    return x


def _same(a, b, what, skip=()):
    """Two results of one dataclass, bit for bit (the float columns too)."""
    assert type(a) is type(b), what
    for f in dataclasses.fields(a):
        va, vb = getattr(a, f.name), getattr(b, f.name)
        if f.name in skip:
            continue
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), (what, f.name)
        else:
            assert va == vb, (what, f.name, va, vb)


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


@pytest.mark.parametrize("devices,option,rccl", TRANSPORTS, ids=["copy", "rccl"])
def test_window_queries_equal_one_engine(devices, option, rccl):
    base, batch = _query_case()
    n = len(devices)
    shards = [SpanBatch(*[col[batch.trace_w1 % np.uint64(n) == i] for col in batch.columns()]) for i in range(n)]
    with _loaded(Group, devices, dataclasses.replace(QCFG, options=QCFG.options | option)) as g, _loaded(Engine, QCFG) as e:
        assert g.size == n and g.uses_rccl == rccl
        members = []
        for sh in shards if n > 1 else []:  # what each member holds: one engine a shard
            m = Engine(QCFG)
            m.window_advance(base)
            m.ingest(sh)
            members.append(m)
        try:
            got, resident = {}, {}
            for name, call in _queries(base).items():
                got[name] = rg = call(g)
                summed = n > 1 and name in ("window_top", "window_movers")
                _same(rg, call(e), name, skip=SUMMED if summed else ())
                if summed:  # every member's candidates are the series it holds
                    resident[name] = [call(m).n_resident for m in members]
                    assert rg.n_resident == sum(resident[name]), name
            if members:
                # ... and its matches those of them that pass on the merged cells, which one engine's
                # point queries give: an estimate >= 1, a score current * 2 - baseline * 2 >= 1
                held = [m.flush().key_hash for m in members]
                assert [len(h) for h in held] == resident["window_top"] == resident["window_movers"]
                est = lambda a, b, h: e.window_range(a, b, h).errors.astype(np.int64)
                assert got["window_top"].n_matched == sum(int((est(base, base + 3, h) >= 1).sum()) for h in held)
                assert got["window_movers"].n_matched == sum(
                    int((2 * est(base + 2, base + 3, h) - 2 * est(base, base + 1, h) >= 1).sum()) for h in held)
            # the answers are not empty ones
            top, lat = _queries(base)["window_top"](g), _queries(base)["window_latency"](g)
            assert len(top.keys) == 10 and top.error_spans > 100 and lat.count.sum() > 2000
            assert _queries(base)["window_latency_movers"](g).spans_cur > 500
        finally:
            for m in members:
                m.close()


@pytest.mark.parametrize("devices,option,rccl", TRANSPORTS, ids=["copy", "rccl"])
def test_a_failed_window_query_leaves_the_next_one_right(devices, option, rccl):
    """A range one past the ring (SA_ERANGE, found by the members) and k = 0
    (SA_EINVAL, found by the group): the group drains its members' streams
    before it returns either, and the next valid query answers as one engine."""
    base, _ = _query_case()
    valid = _queries(base)
    past, k0 = _queries(base, last=base + 4), _queries(base, k=0)
    with _loaded(Group, devices, dataclasses.replace(QCFG, options=QCFG.options | option)) as g, _loaded(Engine, QCFG) as e:
        assert g.uses_rccl == rccl
        want = {name: call(e) for name, call in valid.items()}
        skip = SUMMED if len(devices) > 1 else ()
        for name in valid:
            if name == "window_read":
                continue
            _raises(_lib.SA_ERANGE, lambda: past[name](g))
            assert "member" in g.lib.sa_group_last_error(g._h).decode(), name  # reported as a member's error
            _same(valid[name](g), want[name], (name, "after SA_ERANGE"), skip)
            if name in ("window_top", "window_movers", "window_latency_movers"):
                _raises(_lib.SA_EINVAL, lambda: k0[name](g))
                _same(valid[name](g), want[name], (name, "after SA_EINVAL"), skip)
        for name in valid:  # and every query after every failure
            _same(valid[name](g), want[name], (name, "at the end"), skip)
