"""Error onset over the window ring (sa_window_error_onset,
sa_group_window_error_onset) against the CPU oracle: the candidates are the
series resident in the key table, a split's two estimates are the point queries
on the cells summed over each side, its score the movers', the best split the
largest score and the latest among equal ones -- keys, onsets, scores,
estimates and counters compared with == (tests/error_onset_util.py builds the
cases and the reference; tests/test_window_error_onset_host.py holds the
reference against sketch.error_onset and the crafted cases against their
hand-written answers).

  * a count-min of 2 x 4 where a key's "before" and "after" come from
    different rows; crafted step series;
  * ranges of 1, 2, 3, 8 windows (and 4, 5, 6: the walk takes four windows'
    gathers at a time over the n - 1 splits) on a wrapped ring of 8, of 63,
    64, 65, 128 on a ring of 128, the whole of a ring of 1,024;
  * the select: a cut inside a tie class with more than 4,096 matches, every
    candidate tied, min_count and min_score;
  * a reclaimed table, a full table; every ingest path on a moved ring, an
    unsynchronised device ingest directly before the call;
  * the 2^19-slot binned and dense-ids engines with 64 KiB and 2 MiB of cells;
  * every row against window_range over its two sides and window_movers;
  * groups of two and three members over both transports; the error returns.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import error_onset_util as eu
import keytable_util as kt
import pyoracle
from error_onset_util import assert_onset_equal, candidates, case, onset, reference
from geometry_util import ring_start
from ring_util import DeviceFeed, in_ring
from spanagg import Config, Engine, Group, SpanAggError, SpanBatch, TOP_MAX_K, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

pytestmark = pytest.mark.gpu


def _loaded(name):
    """A fresh engine of the case's config after the case's steps (host
    ingest), the case and the candidates."""
    c = case(name)
    e = Engine(c.cfg)
    try:
        for base, batch in c.steps:
            e.window_advance(base)
            e.ingest(batch)
    except BaseException:
        e.close()
        raise
    return e, c, candidates([b for _, b in c.steps])


def _check(e, c, cand, first, last, ks=(10,), min_count=1, min_score=1, falls=(False, True)):
    windows = reference(c.name)
    for fall in falls:
        for k in ks:
            r = e.window_error_onset(first, last, k, min_count, min_score, fall)
            assert (r.first_window, r.last_window, r.fall) == (first, last, fall)
            assert_onset_equal(r, onset(windows, first, last, cand, k, min_count, min_score, fall),
                               (c.name, first, last, k, min_count, min_score, fall))
    return r


def _consistent(e, r):
    """Every row against the range queries over its two sides and against
    window_movers for that split."""
    first, last = r.first_window, r.last_window
    for t in np.unique(r.onset_window):
        at = np.flatnonzero(r.onset_window == t)
        base, cur = (first, int(t) - 1), (int(t), last)
        keys = r.keys[at]
        assert np.array_equal(e.window_range(*base, keys).errors, r.errors_before[at]), t
        assert np.array_equal(e.window_range(*cur, keys).errors, r.errors_after[at]), t
        m = e.window_movers(base, cur, TOP_MAX_K, fall=r.fall)
        score = dict(zip(m.keys.tolist(), m.score.tolist()))
        assert [score[k] for k in keys.tolist()] == r.score[at].tolist(), t


def test_before_and_after_from_different_rows():
    e, c, cand = _loaded("collide")
    with e:
        assert (c.cfg.cms_d, c.cfg.cms_w) == (2, 4)
        (first, last), = c.ranges
        K, X, Y = eu.collide_keys()
        r = _check(e, c, cand, first, last, (10,), falls=(False,))
        assert eu.items(r) == [(Y, first + 4, 160, 0, 40), (K, first + 2, 40, 2, 26)]
        _consistent(e, r)
        _consistent(e, _check(e, c, cand, first, last, (10,), falls=(True,)))


def test_crafted_step_series():
    e, c, cand = _loaded("steps")
    with e:
        (first, last), = c.ranges
        key = eu.step_keys()
        rise = _check(e, c, cand, first, last, (10, TOP_MAX_K), falls=(False,))
        assert eu.items(rise) == [(key["gap"], first + 5, 45, 0, 9), (key["last"], first + 7, 35, 0, 5),
                                  (key["tie"], first + 7, 12, 2, 2)]
        fall = _check(e, c, cand, first, last, (10,), falls=(True,))
        assert eu.items(fall) == [(key["first"], first + 1, 35, 5, 0), (key["tie"], first + 1, 4, 1, 3)]
        assert (rise.n_resident, rise.n_eligible, rise.n_matched, rise.error_spans) == (6, 5, 3, 39)
        _consistent(e, rise)
        _consistent(e, fall)
        one = _check(e, c, cand, last, last)  # one window: no split
        assert (one.n_resident, one.n_eligible, one.n_matched, one.error_spans, len(one.keys)) == (6, 4, 0, 12, 0)
        assert e.window_error_onset(first, last, 1).items() == rise.items()[:1]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 8])
def test_range_lengths_on_a_wrapped_ring_of_8(n):
    c = case("steps")
    (w0, batch), = c.steps
    cfg, W = c.cfg, c.cfg.n_windows
    base = w0 + 5  # slots 5, 6, 7, 0, 1, 2, 3, 4
    later = eu.craft(cfg, base, [(k, j, (j * i) % 4, 1) for i, k in enumerate(eu.step_keys().values()) for j in range(3, W)], 1)
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(in_ring(batch, cfg, w0))
    o.ingest(later)
    windows = {w: o.window(w) for w in range(base, base + W)}
    cand = candidates([batch])
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(batch)
        e.window_advance(base)
        e.ingest(later)
        for first in sorted({base, min(base + 1, base + W - n), base + W - n}):
            for fall in (False, True):
                r = e.window_error_onset(first, first + n - 1, TOP_MAX_K, fall=fall)
                assert_onset_equal(r, onset(windows, first, first + n - 1, cand, TOP_MAX_K, fall=fall), (n, first, fall))
                assert n > 1 or (r.n_matched, len(r.keys)) == (0, 0)


@pytest.mark.parametrize("name,lengths", [("long128", (63, 64, 65, 128)), ("long1024", (1024,))])
def test_long_rings(name, lengths):
    e, c, cand = _loaded(name)
    with e:
        W = c.cfg.n_windows
        assert W == lengths[-1] and c.base & (W - 1)  # the ring wraps inside the range
        for n in lengths:
            first = c.base + (W - n) // 2
            r = _check(e, c, cand, first, first + n - 1, (10, TOP_MAX_K))
            assert r.n_matched > 10
        _consistent(e, e.window_error_onset(c.base, c.base + W - 1, 3))


def test_the_cut_inside_a_tie_class_with_more_matches_than_the_sort_holds():
    e, c, cand = _loaded("ties_binned")
    with e:
        (first, last), = c.ranges
        assert last > first
        r = _check(e, c, cand, first, last, (10, 3000, TOP_MAX_K), falls=(False,))
        assert r.n_matched > TOP_MAX_K and r.score[-1] == r.score[-300]


@pytest.mark.parametrize("k", [1, 7, 300, TOP_MAX_K])
def test_every_candidate_tied(k):
    e, c, cand = _loaded("all_tied")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (k,), falls=(False,))
        assert np.array_equal(r.keys, np.sort(cand)[:k]) and set(r.score.tolist()) == {45} and r.n_matched == 300


def test_min_count_and_min_score():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        windows = reference(c.name)
        every = onset(windows, first, last, cand, len(cand))
        E = eu.splits(eu.window_cells(windows, first, last), cand)[0]
        mc, ms = int(np.median(E[E > 0])), int(np.median(every.score))
        want = onset(windows, first, last, cand, TOP_MAX_K, mc, ms)
        assert 0 < want.n_matched < want.n_eligible < want.n_resident
        assert want.n_eligible < every.n_eligible and want.n_matched < onset(windows, first, last, cand, 1, mc).n_matched
        r = _check(e, c, cand, first, last, (10, TOP_MAX_K), mc, ms)
        assert int(r.score.min()) >= ms
        _check(e, c, cand, first, last, (TOP_MAX_K,), 0, 0)
        for huge in (2**63 - 1, 2**63, 2**64 - 1):
            r = e.window_error_onset(first, last, 10, min_score=huge)
            assert (len(r.keys), r.n_matched, r.n_eligible, r.n_resident) == (0, 0, every.n_eligible, len(cand)), huge
        r = e.window_error_onset(first, last, 10, min_count=2**64 - 1)
        assert (len(r.keys), r.n_matched, r.n_eligible, r.error_spans) == (0, 0, 0, every.error_spans)


def test_reclaim_empties_the_candidates_and_keeps_the_cells():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        before = _check(e, c, cand, first, last, (10,), falls=(False,))
        e.flush()
        e.reclaim_keys(force=True)
        r = e.window_error_onset(first, last, 10)
        assert (r.n_resident, r.n_eligible, r.n_matched, len(r.keys)) == (0, 0, 0, 0)
        assert r.error_spans == before.error_spans > 0


def test_full_table():
    """kt_default three keys over: the candidates are the rows the flush then
    reports; the dropped series are absent though every one has ERROR spans in
    the cells."""
    row = "kt_default"
    cfg = Config(**kt.KT_ROWS[row]["cfg"])
    w0, cap = ring_start(cfg), kt.cap_of(row)
    keys = kt.full_keys(row, extra=3)
    b = kt.workload(np.random.default_rng(7), kt.spans_for(len(keys)), cfg, keys, w0)
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(in_ring(b, cfg, w0))
    zero = (None, np.zeros((cfg.cms_d, cfg.cms_w), np.uint32))
    seen = set(o.window_ids())
    windows = {w: o.window(w) if w in seen else zero for w in range(w0, w0 + cfg.n_windows)}
    first, last = w0, w0 + cfg.n_windows - 1
    assert last > first
    with Engine(cfg) as e:
        kt.assert_kt_geometry(e, row)
        e.window_advance(w0)
        e.ingest(b)
        r = e.window_error_onset(first, last, TOP_MAX_K)
        res = e.flush(allow_drops=True)
        assert res.status == _lib.SA_EFULL and len(res.key_hash) == cap
        missing = np.setdiff1d(keys, res.key_hash)
        assert len(missing) == 3 and not np.isin(missing, r.keys).any()
        assert_onset_equal(r, onset(windows, first, last, res.key_hash, TOP_MAX_K), "full table")
        assert r.n_resident == cap and r.n_matched > 0


@pytest.mark.parametrize("mode", ["host", "device", "many"])
def test_every_ingest_path_on_a_moved_ring(mode):
    """The steps of moved:ring_512 through the ring walk's feeds: host ingest,
    device streams, ingest_device_many -- the device ones unsynchronised, the
    last launch directly before the call."""
    c, windows = case("moved:ring_512"), reference("moved:ring_512")
    (b0, first_batch), (b1, second) = c.steps
    cand = candidates([first_batch, second])
    W = c.cfg.n_windows
    with Engine(c.cfg) as e:
        if mode == "host":
            feed = lambda name: e.ingest(dict(A=first_batch, B=second)[name])
        else:
            feed = DeviceFeed(e, SimpleNamespace(batches=dict(A=first_batch, B=second), row="window_error_onset"),
                              graph=mode == "many")
        e.window_advance(b0)
        feed("A")
        e.window_advance(b1)
        feed("B")
        r = e.window_error_onset(b1, b1 + W - 1, TOP_MAX_K)
        assert_onset_equal(r, onset(windows, b1, b1 + W - 1, cand, TOP_MAX_K), mode)
        assert r.n_matched > 10
        again = e.window_error_onset(b1, b1 + W - 1, TOP_MAX_K)
        assert again.items() == r.items()
        assert (again.n_resident, again.n_eligible, again.n_matched, again.error_spans) == \
            (r.n_resident, r.n_eligible, r.n_matched, r.error_spans)
        for first, last in c.ranges:
            for fall in (False, True):
                got = e.window_error_onset(first, last, 10, fall=fall)
                assert_onset_equal(got, onset(windows, first, last, cand, 10, fall=fall), (mode, first, last, fall))
        for w in range(b1, b1 + W):  # the query folded what it read and cleared nothing
            sk = e.window_read(w)
            assert np.array_equal(sk.hll, windows[w][0]) and np.array_equal(sk.cms, windows[w][1]), w


@pytest.mark.parametrize("name", ["full:ring_binned", "full:ring_dense", "binned_w64k", "dense_w64k"])
def test_large_tables_on_both_sides_of_the_staged_cells(name):
    e, c, cand = _loaded(name)
    with e:
        assert e.stats()["table_capacity"] == 1 << 19
        assert c.cfg.cms_d * c.cfg.cms_w * 8 == (1 << 21 if name.endswith("w64k") else 1 << 16)
        (first, last), = c.ranges
        r = _check(e, c, cand, first, last, (10, TOP_MAX_K))
        assert r.n_matched > 10 and r.n_resident == len(cand)
        _consistent(e, e.window_error_onset(first, last, 5))


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def test_errors_leave_the_engine_usable():
    e, c, cand = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        W = c.cfg.n_windows
        out = C.POINTER(_lib.sa_error_onset_result)()
        call = lambda k, flags, o=out: e.lib.sa_window_error_onset(e._h, first, last, k, 1, 1, flags, C.byref(o))
        assert call(0, 0) == _lib.SA_EINVAL and not out
        assert call(TOP_MAX_K + 1, 0) == _lib.SA_EINVAL and not out
        assert call(10, 2) == _lib.SA_EINVAL and not out
        assert call(10, _lib.SA_ERROR_ONSET_FALL | 4) == _lib.SA_EINVAL and not out
        assert e.lib.sa_window_error_onset(e._h, first, last, 10, 1, 1, 0, None) == _lib.SA_EINVAL
        _raises(_lib.SA_EINVAL, lambda: e.window_error_onset(first, last, 0))
        for a, b in ((first + 1, first), (first - 1, last), (first, first + W), (first + W, first + W)):
            _raises(_lib.SA_ERANGE, lambda: e.window_error_onset(a, b))
        _check(e, c, cand, first, last, (10, TOP_MAX_K))


@pytest.mark.parametrize("devices,option,rccl", [([0, 0], OPT_GROUP_COPY, False), ([0, 0, 0], OPT_GROUP_COPY, False),
                                                 ([0], OPT_GROUP_RCCL, True), ([0, 0, 0], OPT_GROUP_RCCL, False)])
def test_group_equals_the_oracle_and_one_engine(devices, option, rccl):
    """The device/option rows of the movers' group test, and two members over
    the copy transport."""
    c, windows = case("group"), reference("group")
    (ring_base, batch), = c.steps
    first, last = ring_base + 1, ring_base + 6
    cand = candidates([batch])
    n = len(devices)
    shards = [candidates([SpanBatch(*[col[batch.trace_w1 % np.uint64(n) == i] for col in batch.columns()])])
              for i in range(n)]
    assert n == 1 or sum(len(s) for s in shards) > len(cand)  # series on several members
    with Group(devices, dataclasses.replace(c.cfg, options=option)) as g, Engine(c.cfg) as e:
        assert g.size == n and g.uses_rccl == rccl
        for x in (g, e):
            x.window_advance(ring_base)
            x.ingest(batch)
        for fall in (False, True):
            for k in (10, TOP_MAX_K):
                want = onset(windows, first, last, cand, k, fall=fall)
                assert want.n_matched > 10
                one = (len(cand), want.n_eligible, want.n_matched)
                per = [onset(windows, first, last, s, k, fall=fall) for s in shards]
                want.n_resident, want.n_eligible = sum(p.n_resident for p in per), sum(p.n_eligible for p in per)
                want.n_matched = sum(p.n_matched for p in per)
                rg = g.window_error_onset(first, last, k, fall=fall)
                assert_onset_equal(rg, want, ("group", k, fall))
                assert len(set(rg.keys.tolist())) == len(rg.keys)  # a series on two members: once
                re_ = e.window_error_onset(first, last, k, fall=fall)
                assert re_.items() == rg.items() and re_.error_spans == rg.error_spans
                assert (re_.n_resident, re_.n_eligible, re_.n_matched) == one
        one_window = g.window_error_onset(first, first, 10)
        assert (one_window.n_matched, len(one_window.keys)) == (0, 0) and one_window.n_eligible > 0
        _raises(_lib.SA_ERANGE, lambda: g.window_error_onset(ring_base, ring_base + c.cfg.n_windows))
        _raises(_lib.SA_ERANGE, lambda: g.window_error_onset(ring_base + 2, ring_base + 1))
        _raises(_lib.SA_EINVAL, lambda: g.window_error_onset(first, last, 0))
        # the range queries after it still answer as the oracle
        rr = g.window_range(first, last, rg.keys, cells=True)
        assert np.array_equal(rr.cms, eu.window_cells(windows, first, last).sum(axis=0))
