"""Heavy hitters over the window ring (sa_window_top, sa_group_window_top)
against the CPU oracle: the candidates are the series resident in the key
table, the estimate is the point query on the cells summed over first..last,
the order is sketch.heavy_hitters' -- keys, estimates and counters compared
with == (tests/top_util.py builds the cases and the references;
tests/test_window_top_host.py proves the inputs can catch a wrong tie-break, a
wrong range and a missing candidate filter).

  * every row of RING_ROWS (every ingest path), k = 10 and k = SA_TOP_MAX_K;
    every estimate is window_range's for that key;
  * ties: a count-min of two cells (two classes of the whole table), and a
    binned table whose cut falls inside a class of thousands;
  * cells of 128 KiB, 256 KiB and 1 MiB beside the default 64 KiB and the
    16 bytes of the tie case;
  * tables of 4,096 slots (the select never has work) and of 8,192 with more
    than 4,096 matches (it has);
  * every sub-range of a moved ring;
  * min_count; a reclaimed table; a full table; idempotence and ordering
    behind an unsynchronised device ingest; the error returns;
  * groups of three members and of one, over both transports.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import keytable_util as kt
import pyoracle
import top_util
from geometry_util import RING_ROWS, assert_geometry, ring_start
from ring_util import DeviceFeed, in_ring
from spanagg import Config, Engine, Group, SpanAggError, SpanBatch, TOP_MAX_K, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL
from top_util import assert_top_equal, candidates, case, cells, reference, top

pytestmark = pytest.mark.gpu


def _loaded(name):
    """A fresh engine of the case's config after the case's steps (host
    ingest), the case and the candidates."""
    c = case(name)
    e = Engine(c.cfg)
    try:
        if c.row:
            assert_geometry(e, c.row)
        for base, batch in c.steps:
            e.window_advance(base)
            e.ingest(batch)
    except BaseException:
        e.close()
        raise
    return e, c, candidates([b for _, b in c.steps])


def _check(e, c, cand, first, last, ks, min_count=1):
    cms = cells(reference(c.name), first, last)
    for k in ks:
        r = e.window_top(first, last, k, min_count)
        assert (r.first, r.last) == (first, last)
        assert_top_equal(r, top(cms, cand, k, min_count), (c.name, first, last, k, min_count))
    return r


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_full_ring_on_every_path(row):
    e, c, cand = _loaded(f"full:{row}")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (10, TOP_MAX_K))
        assert len(r.keys) == min(r.n_matched, TOP_MAX_K) > 10
        # every estimate is the range query's for that key, the counters the engine's own
        rr = e.window_range(first, last, r.keys, cells=True)
        assert np.array_equal(rr.errors, r.errors)
        assert r.error_spans == int(rr.cms[0].sum())
        assert r.items() == rr.top_errors(len(r.keys))
        assert r.n_resident == e.stats()["n_keys"] == len(cand)


@pytest.mark.parametrize("k", top_util.TIES_SMALL_KS)
def test_two_tie_classes_of_the_whole_table(k):
    e, c, cand = _loaded("ties_small")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (k,))
        assert len(r.keys) == min(k, len(cand)) and len(np.unique(r.errors)) <= 2


def test_the_cut_inside_a_tie_class_of_thousands():
    e, c, cand = _loaded("ties_binned")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (10, top_util.TIES_BINNED_K, TOP_MAX_K))
        assert r.n_matched > 10 * TOP_MAX_K and r.errors[-1] == r.errors[-1000]


@pytest.mark.parametrize("name", list(top_util.CELL_SIZES))
def test_cell_sizes(name):
    e, c, cand = _loaded(name)
    with e:
        assert (c.cfg.cms_d, c.cfg.cms_w) == top_util.CELL_SIZES[name]
        (first, last), = c.ranges
        _check(e, c, cand, first, last, (10, TOP_MAX_K))
        _check(e, c, cand, first, first, (10,))


@pytest.mark.parametrize("name,slots", [("slots4096", 4096), ("slots8192", 8192)])
def test_table_sizes_on_both_sides_of_the_select(name, slots):
    e, c, cand = _loaded(name)
    with e:
        assert e.stats()["table_capacity"] == slots
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (10, 100, TOP_MAX_K))
        assert (r.n_matched > TOP_MAX_K) == (slots == 8192)


def test_sub_ranges_and_wrap_on_a_moved_ring():
    e, c, cand = _loaded("moved:ring_512")
    with e:
        assert len(c.ranges) == 10
        for first, last in c.ranges:
            _check(e, c, cand, first, last, (10, TOP_MAX_K))


def test_min_count():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        everything = _check(e, c, cand, first, last, (TOP_MAX_K,))
        for j in (0, 9, 40, len(everything.errors) - 1):
            m = int(everything.errors[j])
            r = _check(e, c, cand, first, last, (10, TOP_MAX_K), min_count=m)
            assert r.n_matched == int((everything.errors >= m).sum()) >= j + 1
            assert int(r.errors[-1]) >= m and np.array_equal(r.keys, everything.keys[: r.n_matched])
        above = _check(e, c, cand, first, last, (10,), min_count=int(everything.errors[0]) + 1)
        assert (len(above.keys), above.n_matched, above.n_resident) == (0, 0, len(cand))
        assert above.error_spans == everything.error_spans
        zero = _check(e, c, cand, first, last, (TOP_MAX_K,), min_count=0)
        assert zero.items() == everything.items() and zero.n_matched == everything.n_matched
        huge = e.window_top(first, last, 10, 2**64 - 1)
        assert (len(huge.keys), huge.n_matched) == (0, 0)


def test_reclaim_empties_the_candidates_and_keeps_the_cells():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        cms = cells(reference(c.name), first, last)
        before = _check(e, c, cand, first, last, (10,))
        e.flush()
        e.reclaim_keys(force=True)
        r = e.window_top(first, last, 10)
        assert (r.n_resident, r.n_matched, len(r.keys)) == (0, 0, 0) and r.error_spans == before.error_spans
        key = int(before.keys[0])
        assert int(e.window_range(first, last, [key]).errors[0]) == int(before.errors[0]) > 0
        # a further small batch: exactly its keys are candidates, with the old errors in their estimates
        (base, batch), = c.steps
        ok = np.flatnonzero(((batch.meta >> np.uint32(19)) & np.uint32(3)) != 2)[:40]  # no ERROR span: the cells stay
        few = SpanBatch(*[col[ok] for col in batch.columns()])
        again = candidates([few])
        assert 10 < len(again) < len(cand)
        e.ingest(few)
        r = e.window_top(first, last, TOP_MAX_K)
        assert_top_equal(r, top(cms, again, TOP_MAX_K), "after the reclaim")
        assert int(r.errors[0]) > 40  # more than the batch could have added


def test_full_table():
    """kt_default three keys over: the candidates are the rows the flush then
    reports; the dropped series are absent though every one has an ERROR span
    in the cells."""
    row = "kt_default"
    cfg = Config(**kt.KT_ROWS[row]["cfg"])
    w0, cap = ring_start(cfg), kt.cap_of(row)
    keys = kt.full_keys(row, extra=3)
    b = kt.workload(np.random.default_rng(7), kt.spans_for(len(keys)), cfg, keys, w0)
    # one ERROR span on every key, in the ring and on a valid service
    w = b.end_ns // np.uint64(cfg.window_ns)
    fit = np.flatnonzero((w >= w0) & (w < w0 + cfg.n_windows) & ((b.meta & np.uint32(0xFFFF)) < cfg.n_services))
    fit = fit[: len(keys)]
    assert len(fit) == len(keys)
    cols = [col[fit].copy() for col in b.columns()]
    cols[0] = keys.copy()
    cols[5] = (cols[5] & ~np.uint32(3 << 19)) | np.uint32(2 << 19)
    errs = SpanBatch(*cols)
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(in_ring(b, cfg, w0))
    o.ingest(errs)
    cms = np.sum([o.window(wid)[1].astype(np.uint64) for wid in o.window_ids()], axis=0, dtype=np.uint64)
    with Engine(cfg) as e:
        kt.assert_kt_geometry(e, row)
        e.window_advance(w0)
        e.ingest(b)
        e.ingest(errs)
        r = e.window_top(w0, w0 + cfg.n_windows - 1, TOP_MAX_K)
        res = e.flush(allow_drops=True)
        assert res.status == _lib.SA_EFULL and len(res.key_hash) == cap
        missing = np.setdiff1d(keys, res.key_hash)
        assert len(missing) == 3 and not np.isin(missing, r.keys).any()
        assert (top_util.estimates(cms, missing) >= 1).all()  # they would have matched
        assert_top_equal(r, top(cms, res.key_hash, TOP_MAX_K), "full table")
        assert r.n_resident == r.n_matched == cap == len(r.keys)
        assert r.error_spans == int(cms[0].sum()) >= len(keys)


def test_idempotent_and_ordered_behind_a_device_ingest():
    c, windows = case("full:ring_512"), reference("full:ring_512")
    (base, batch), = c.steps
    (first, last), = c.ranges
    cand, cms = candidates([batch]), cells(windows, first, last)
    with Engine(c.cfg) as e:
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_top"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_top(first, last, TOP_MAX_K)
        assert_top_equal(r, top(cms, cand, TOP_MAX_K), "behind the ingest")
        again = e.window_top(first, last, TOP_MAX_K)
        assert again.items() == r.items()
        assert (again.n_resident, again.n_matched, again.error_spans) == (r.n_resident, r.n_matched, r.error_spans)
        rr = e.window_range(first, last, r.keys, cells=True)
        assert np.array_equal(rr.cms, cms) and np.array_equal(rr.errors, r.errors)
        for w in range(first, last + 1):
            sk = e.window_read(w)
            assert np.array_equal(sk.hll, windows[w][0]) and np.array_equal(sk.cms, windows[w][1]), w
        assert e.window_top(first, last, TOP_MAX_K).items() == r.items()


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def test_errors_leave_the_engine_usable():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        W = c.cfg.n_windows
        out = C.POINTER(_lib.sa_top_result)()
        call = lambda k, flags, o=out: e.lib.sa_window_top(e._h, first, last, k, 1, flags, C.byref(o))
        assert call(0, 0) == _lib.SA_EINVAL and not out
        assert call(TOP_MAX_K + 1, 0) == _lib.SA_EINVAL and not out
        assert call(10, 1) == _lib.SA_EINVAL and not out
        assert e.lib.sa_window_top(e._h, first, last, 10, 1, 0, None) == _lib.SA_EINVAL
        _raises(_lib.SA_EINVAL, lambda: e.window_top(first, last, 0))
        _raises(_lib.SA_ERANGE, lambda: e.window_top(first + 1, first))
        _raises(_lib.SA_ERANGE, lambda: e.window_top(first - 1, last))
        _raises(_lib.SA_ERANGE, lambda: e.window_top(first, first + W))
        _check(e, c, cand, first, last, (10, TOP_MAX_K))


@pytest.mark.parametrize("devices,option,rccl", [([0, 0, 0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True),
                                                 ([0, 0, 0], OPT_GROUP_RCCL, False)])
def test_group_equals_the_oracle_and_one_engine(devices, option, rccl):
    """Three members over the copy transport; RCCL where a communicator can be
    had on one device (a group of one); and three members that ask for RCCL
    on one device, which a communicator cannot hold: the copy transport."""
    c, windows = case("group"), reference("group")
    (base, batch), = c.steps
    (first, last), = c.ranges
    cand, cms = candidates([batch]), cells(windows, first, last)
    n = len(devices)
    shards = [candidates([SpanBatch(*[col[batch.trace_w1 % np.uint64(n) == i] for col in batch.columns()])])
              for i in range(n)]
    assert n == 1 or sum(len(s) for s in shards) > len(cand)  # series on several members
    with Group(devices, dataclasses.replace(c.cfg, options=option)) as g, Engine(c.cfg) as e:
        assert g.size == n and g.uses_rccl == rccl
        for x in (g, e):
            x.window_advance(base)
            x.ingest(batch)
        for k in (10, TOP_MAX_K):
            want = top(cms, cand, k)
            per = [top(cms, s, k) for s in shards]
            want.n_resident, want.n_matched = sum(p.n_resident for p in per), sum(p.n_matched for p in per)
            rg = g.window_top(first, last, k)
            assert_top_equal(rg, want, ("group", k))
            re_ = e.window_top(first, last, k)
            assert re_.items() == rg.items() and re_.error_spans == rg.error_spans
            assert (re_.n_resident, re_.n_matched) == (len(cand), top(cms, cand, k).n_matched)
        _raises(_lib.SA_ERANGE, lambda: g.window_top(base, base + c.cfg.n_windows))
        _raises(_lib.SA_EINVAL, lambda: g.window_top(first, last, 0))
        # the range query after it still answers as the oracle
        rr = g.window_range(first, last, rg.keys, cells=True)
        assert np.array_equal(rr.cms, cms) and np.array_equal(rr.errors, rg.errors)
