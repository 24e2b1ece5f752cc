"""Movers over the window ring (sa_window_movers, sa_group_window_movers)
against the CPU oracle: the candidates are the series resident in the key
table, the two estimates are the point queries on the cells summed over each
range, the score is current * n_base - baseline * n_cur in int64, the order is
sketch.movers' -- keys, scores, estimates and counters compared with ==
(tests/movers_util.py builds the cases and the references;
tests/test_window_movers_host.py proves the inputs can catch a wrong tie-break,
a wrong normalisation and a missing baseline).

  * every row of RING_ROWS (every ingest path), the ring's halves, k = 10 and
    k = SA_TOP_MAX_K, rises and falls; every estimate is window_range's;
  * ties: a count-min of two cells, and a binned table whose cuts fall inside
    classes of thousands;
  * two cell arrays of 128 KiB, 256 KiB and 1 MiB each beside the default
    64 KiB (the two together: the most a workgroup stages) and the 16 bytes of
    the tie case;
  * every ordered pair of a moved ring's sub-ranges: unequal lengths, overlap,
    equality, the wrap;
  * a planted incident; min_score; a reclaimed table; idempotence and ordering
    behind an unsynchronised device ingest; the error returns;
  * groups of three members and of one, over both transports.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import movers_util as mu
import top_util
from geometry_util import RING_ROWS, assert_geometry
from movers_util import assert_movers_equal, candidates, case, cells, movers, reference, split
from ring_util import DeviceFeed
from spanagg import Engine, Group, SpanAggError, SpanBatch, TOP_MAX_K, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

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


def _check(e, c, cand, base, cur, ks, min_score=1, falls=(False, True)):
    windows = reference(c.name)
    for fall in falls:
        for k in ks:
            r = e.window_movers(base, cur, k, min_score, fall)
            assert (r.base, r.cur, r.fall) == (base, cur, fall)
            assert_movers_equal(r, movers(windows, base, cur, cand, k, min_score, fall),
                                (c.name, base, cur, k, min_score, fall))
    return r


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_ring_halves_on_every_path(row):
    e, c, cand = _loaded(f"full:{row}")
    with e:
        base, cur = split(c)
        for fall in (False, True):
            r = _check(e, c, cand, base, cur, (10, TOP_MAX_K), falls=(fall,))
            assert len(r.keys) == min(r.n_matched, TOP_MAX_K)
            # every estimate is the range query's for that key, the counters the engine's own
            rb, rc = e.window_range(*base, r.keys, cells=True), e.window_range(*cur, r.keys, cells=True)
            assert np.array_equal(rb.errors, r.baseline) and np.array_equal(rc.errors, r.current)
            assert (r.error_spans_base, r.error_spans_cur) == (int(rb.cms[0].sum()), int(rc.cms[0].sum()))
            assert r.n_resident == e.stats()["n_keys"] == len(cand)
            if c.cfg.n_windows == 1:  # equal ranges: nothing moved
                assert base == cur and (r.n_matched, len(r.keys)) == (0, 0)
                assert r.error_spans_base == r.error_spans_cur > 0
            else:
                assert len(r.keys) > 10 and (r.score >= 1).all()
                sign = -1 if fall else 1
                nb, nc = base[1] - base[0] + 1, cur[1] - cur[0] + 1
                assert np.array_equal(r.score, sign * (r.current.astype(np.int64) * nb - r.baseline.astype(np.int64) * nc))


@pytest.mark.parametrize("k", top_util.TIES_SMALL_KS)
def test_two_cells_for_the_whole_table(k):
    e, c, cand = _loaded("ties_small")
    with e:
        base, cur = split(c)
        assert (c.cfg.cms_d, c.cfg.cms_w) == (1, 2)
        r = _check(e, c, cand, base, cur, (k,))  # the whole table fell ...
        assert len(r.keys) == min(k, len(cand)) and len(np.unique(r.score)) <= 2
        r = _check(e, c, cand, cur, base, (k,), falls=(False,))  # ... or rose
        assert len(r.keys) == min(k, len(cand)) and len(np.unique(r.score)) <= 2


def test_the_cuts_inside_tie_classes_of_thousands():
    e, c, cand = _loaded("ties_binned")
    with e:
        base, cur = split(c)
        r = _check(e, c, cand, base, cur, (10, top_util.TIES_BINNED_K, TOP_MAX_K))
        assert r.n_matched > 4 * TOP_MAX_K and r.score[-1] == r.score[-300]


@pytest.mark.parametrize("name", list(top_util.CELL_SIZES))
def test_cell_sizes(name):
    e, c, cand = _loaded(name)
    with e:
        assert (c.cfg.cms_d, c.cfg.cms_w) == top_util.CELL_SIZES[name]
        base, cur = split(c)
        r = _check(e, c, cand, base, cur, (10, TOP_MAX_K))
        assert r.n_matched > 100
        whole = (base[0], cur[1])
        _check(e, c, cand, whole, cur, (10,))


def test_every_ordered_pair_of_sub_ranges_on_a_moved_ring():
    e, c, cand = _loaded("moved:ring_512")
    with e:
        assert len(c.ranges) == 10
        for i, base in enumerate(c.ranges):
            for j, cur in enumerate(c.ranges):
                r = _check(e, c, cand, base, cur, (TOP_MAX_K,), falls=(False,))
                assert base != cur or (r.n_matched, r.error_spans_base) == (0, r.error_spans_cur)
                if (i + j) % 7 == 0:
                    _check(e, c, cand, base, cur, (10,), falls=(True,))


def test_wrap_ranges_against_the_full_ring():
    e, c, cand = _loaded("moved:ring_1024_noerr")
    with e:
        W = c.cfg.n_windows
        full = (c.base, c.base + W - 1)
        assert full in c.ranges and len(c.ranges) == 6
        for rng in c.ranges:
            _check(e, c, cand, full, rng, (10, TOP_MAX_K))
            _check(e, c, cand, rng, full, (TOP_MAX_K,), falls=(False,))


def test_planted_incident():
    e, c, cand = _loaded("planted")
    with e:
        base, cur = split(c)
        r = _check(e, c, cand, base, cur, (10,), falls=(False,))
        assert set(r.keys[:3]) == set(mu.planted_keys())
        assert [int(s) for s in r.score[:4]] == [2755, 2755, 2595, 31] and r.keys[0] < r.keys[1]
        back = _check(e, c, cand, cur, base, (10,), falls=(True,))
        assert np.array_equal(back.keys, r.keys) and np.array_equal(back.score, r.score)
        assert np.array_equal(back.baseline, r.current) and np.array_equal(back.current, r.baseline)


def test_min_score():
    e, c, cand = _loaded("full:ring_512")
    with e:
        base, cur = split(c)
        everything = _check(e, c, cand, base, cur, (TOP_MAX_K,), falls=(False,))
        for j in (0, 9, 40, len(everything.score) - 1):
            m = int(everything.score[j])
            r = _check(e, c, cand, base, cur, (10, TOP_MAX_K), min_score=m, falls=(False,))
            assert r.n_matched == int((everything.score >= m).sum()) >= j + 1
            assert int(r.score[-1]) >= m and np.array_equal(r.keys, everything.keys[: r.n_matched])
        above = _check(e, c, cand, base, cur, (10,), min_score=int(everything.score[0]) + 1, falls=(False,))
        assert (len(above.keys), above.n_matched, above.n_resident) == (0, 0, len(cand))
        assert (above.error_spans_base, above.error_spans_cur) == (everything.error_spans_base, everything.error_spans_cur)
        zero = _check(e, c, cand, base, cur, (TOP_MAX_K,), min_score=0, falls=(False,))
        assert zero.items() == everything.items() and zero.n_matched == everything.n_matched
        for huge in (2**63 - 1, 2**63, 2**64 - 1):
            for fall in (False, True):
                r = e.window_movers(base, cur, 10, huge, fall)
                assert (len(r.keys), r.n_matched, r.n_resident) == (0, 0, len(cand)), (huge, fall)


def test_reclaim_empties_the_candidates_and_keeps_the_cells():
    e, c, cand = _loaded("full:ring_512")
    with e:
        base, cur = split(c)
        before = _check(e, c, cand, base, cur, (10,), falls=(False,))
        e.flush()
        e.reclaim_keys(force=True)
        r = e.window_movers(base, cur, 10)
        assert (r.n_resident, r.n_matched, len(r.keys)) == (0, 0, 0)
        assert (r.error_spans_base, r.error_spans_cur) == (before.error_spans_base, before.error_spans_cur)
        # a further small batch: exactly its keys are candidates, with the old errors in their estimates
        (_, batch), = c.steps
        ok = np.flatnonzero(((batch.meta >> np.uint32(19)) & np.uint32(3)) != 2)[:40]  # no ERROR span: the cells stay
        few = SpanBatch(*[col[ok] for col in batch.columns()])
        again = candidates([few])
        assert 10 < len(again) < len(cand)
        e.ingest(few)
        for fall in (False, True):
            r = e.window_movers(base, cur, TOP_MAX_K, fall=fall)
            assert_movers_equal(r, movers(reference(c.name), base, cur, again, TOP_MAX_K, fall=fall), "after the reclaim")
            assert r.n_resident == len(again)


def test_idempotent_and_ordered_behind_a_device_ingest():
    c, windows = case("full:ring_512"), reference("full:ring_512")
    (ring_base, batch), = c.steps
    (first, last), = c.ranges
    base, cur = split(c)
    cand = candidates([batch])
    with Engine(c.cfg) as e:
        e.window_advance(ring_base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_movers"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_movers(base, cur, TOP_MAX_K)
        assert_movers_equal(r, movers(windows, base, cur, cand, TOP_MAX_K), "behind the ingest")
        again = e.window_movers(base, cur, TOP_MAX_K)
        assert again.items() == r.items()
        assert (again.n_resident, again.n_matched, again.error_spans_base, again.error_spans_cur) == \
            (r.n_resident, r.n_matched, r.error_spans_base, r.error_spans_cur)
        for w in range(first, last + 1):
            sk = e.window_read(w)
            assert np.array_equal(sk.hll, windows[w][0]) and np.array_equal(sk.cms, windows[w][1]), w
        whole = cells(windows, first, last)
        top_util.assert_top_equal(e.window_top(first, last, TOP_MAX_K), top_util.top(whole, cand, TOP_MAX_K), "top after")
        assert e.window_movers(base, cur, TOP_MAX_K).items() == r.items()


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def test_errors_leave_the_engine_usable():
    e, c, cand = _loaded("full:ring_512")
    with e:
        base, cur = split(c)
        (first, last), = c.ranges
        W = c.cfg.n_windows
        out = C.POINTER(_lib.sa_movers_result)()
        call = lambda k, flags, o=out: e.lib.sa_window_movers(e._h, base[0], base[1], cur[0], cur[1], k, 1, flags, C.byref(o))
        assert call(0, 0) == _lib.SA_EINVAL and not out
        assert call(TOP_MAX_K + 1, 0) == _lib.SA_EINVAL and not out
        assert call(10, 2) == _lib.SA_EINVAL and not out
        assert call(10, _lib.SA_MOVERS_FALL | 4) == _lib.SA_EINVAL and not out
        assert e.lib.sa_window_movers(e._h, base[0], base[1], cur[0], cur[1], 10, 1, 0, None) == _lib.SA_EINVAL
        _raises(_lib.SA_EINVAL, lambda: e.window_movers(base, cur, 0))
        for bad in ((first + 1, first), (first - 1, last), (first, first + W)):
            _raises(_lib.SA_ERANGE, lambda: e.window_movers(bad, cur))
            _raises(_lib.SA_ERANGE, lambda: e.window_movers(base, bad))
        _check(e, c, cand, base, cur, (10, TOP_MAX_K))


@pytest.mark.parametrize("devices,option,rccl", [([0, 0, 0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True),
                                                 ([0, 0, 0], OPT_GROUP_RCCL, False)])
def test_group_equals_the_oracle_and_one_engine(devices, option, rccl):
    """The device/option rows of the heavy hitters' group test: three members
    over the copy transport; RCCL on a group of one; three members that ask
    for RCCL on one device, which a communicator cannot hold."""
    c, windows = case("group"), reference("group")
    (ring_base, batch), = c.steps
    base, cur = (ring_base + 1, ring_base + 3), (ring_base + 4, ring_base + 5)
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
                want = movers(windows, base, cur, cand, k, fall=fall)
                assert want.n_matched > 10
                one = (len(cand), want.n_matched)
                per = [movers(windows, base, cur, s, k, fall=fall) for s in shards]
                want.n_resident, want.n_matched = sum(p.n_resident for p in per), sum(p.n_matched for p in per)
                rg = g.window_movers(base, cur, k, fall=fall)
                assert_movers_equal(rg, want, ("group", k, fall))
                re_ = e.window_movers(base, cur, k, fall=fall)
                assert re_.items() == rg.items()
                assert (re_.error_spans_base, re_.error_spans_cur) == (rg.error_spans_base, rg.error_spans_cur)
                assert (re_.n_resident, re_.n_matched) == one
        _raises(_lib.SA_ERANGE, lambda: g.window_movers((ring_base, ring_base + c.cfg.n_windows), cur))
        _raises(_lib.SA_ERANGE, lambda: g.window_movers(base, (ring_base + 2, ring_base + 1)))
        _raises(_lib.SA_EINVAL, lambda: g.window_movers(base, cur, 0))
        # the range queries after it still answer as the oracle
        for rng in (base, cur):
            rr = g.window_range(*rng, rg.keys, cells=True)
            assert np.array_equal(rr.cms, cells(windows, *rng))
            assert np.array_equal(rr.errors, rg.baseline if rng == base else rg.current)
