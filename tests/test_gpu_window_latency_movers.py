"""sa_window_latency_movers on the GPU (spanagg_latency.hip, the select of
spanagg_range.hip) against the numpy restatement of tests/latency_movers_util.py;
every comparison is ==, and every case asserts the property it was built for.

  crafted shifts, tie cuts, service counts (with the rows held against
  window_latency), ranges on a moved ring, long ranges (both sides of every
  stripe count of the sums kernel), the select path (more matches than the sort
  holds, k = 4,096, 1 and 10; key 0 among them), the 65,536-service ring, the
  scratch shared with window_top, a binned engine, a call behind an
  unsynchronised device ingest, groups of three over both transports, and
  every error return.
"""
import ctypes as C
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import latency_movers_util as mu
import latency_util as lu
import pyoracle
import top_util
from geometry_util import make_batch, ring_start
from ring_util import DeviceFeed, in_ring
from spanagg import Config, Engine, Group, SpanAggError, SpanBatch, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL, OPT_WINDOW_LATENCY

pytestmark = pytest.mark.gpu


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def _check_calls(x, c, calls=None):
    out = []
    for call in calls or c.calls:
        r = mu.run(x, call)
        assert (r.base, r.cur, r.fall) == (call[0], call[1], call[6]) and r.q_ppm.tolist() == list(call[3])
        mu.assert_latency_movers(r, mu.want(c, call), (c.name, call[2:]))
        out.append(r)
    return out


def test_crafted_shifts():
    c = mu.case("crafted")
    with mu.loaded(c) as e:
        rs = _check_calls(e, c)
        rise, fall, cut = rs[0], rs[1], rs[2]
        assert list(zip(rise.services.tolist(), rise.shift.tolist())) == mu.CRAFTED_RISE  # service 0 on top
        assert list(zip(fall.services.tolist(), fall.shift.tolist())) == mu.CRAFTED_FALL  # exactly the negatives
        assert rise.n_eligible == 5 and 3 not in rise.services and 3 not in fall.services  # one range only
        assert cut.services.tolist() == [0, 1] and cut.n_matched == 3
        # min_shift at and above service 1's 30, and above every bin
        assert rs[3].services.tolist() == [0, 1] and rs[4].services.tolist() == [0] and rs[5].n_matched == 0
        # min_count at 3 (services 0 and 4 have 3 spans in the current range), 4 (every baseline has 4) and 5
        assert [r.services.tolist() for r in rs[6:9]] == [[0, 1, 4], [1], []]
        assert [r.n_eligible for r in rs[6:9]] == [4, 2, 0]
        assert [r.services.tolist() for r in rs[9:11]] == [[2], []]
        assert rs[11].q_bin_cur.shape == (len(rs[11].services), 1)  # one quantile


def test_tie_cuts():
    c = mu.case("ties")
    with mu.loaded(c) as e:
        rs = _check_calls(e, c)
        for r, k in zip(rs, mu.TIES_KS):
            assert r.services.tolist() == mu.TIES_ORDER[:k] and r.n_matched == 12
        full = mu.want(c, (c.calls[0][0], c.calls[0][1], 12) + c.calls[0][3:])
        sh, cnt = full.shift.tolist(), full.count_cur.tolist()
        assert sh[4] == sh[5] and cnt[4] > cnt[5] and full.services[4] > full.services[5]  # k = 5: the count decides
        for k in (2, 7, 10):  # the id decides
            assert (sh[k - 1], cnt[k - 1]) == (sh[k], cnt[k]) and full.services[k - 1] < full.services[k]


@pytest.mark.parametrize("S", mu.SERVICE_COUNTS)
def test_service_counts(S):
    c = mu.case(f"services{S}")
    with mu.loaded(c) as e:
        rs = _check_calls(e, c)
        assert rs[0].n_matched >= min(S, 2) // 2 and len(rs[0].services) == min(64, rs[0].n_matched)
        assert rs[0].q_bin_cur.shape == (len(rs[0].services), 3)
        for r, call in zip(rs, c.calls):  # the consistency rule
            for i, s in enumerate(r.services.tolist()):
                for rng_, cnt, qb, qn in ((call[0], r.count_base, r.q_bin_base, r.q_ns_base),
                                          (call[1], r.count_cur, r.q_bin_cur, r.q_ns_cur)):
                    one = e.window_latency(*rng_, services=[s], quantiles=mu.Q3)
                    assert one.count[0, 0] == cnt[i] and np.array_equal(one.q_bin[0, 0], qb[i])
                    assert np.array_equal(one.q_ns[0, 0], qn[i])


def test_ranges_on_a_moved_ring():
    c = mu.case("ranges")
    with mu.loaded(c) as e:
        rs = _check_calls(e, c)
        assert c.base & (c.cfg.n_windows - 1)  # the ring's first window is not slot 0
        assert sum(r.n_matched for r in rs) > 0
        for r in rs[2:4]:  # equal ranges
            assert r.base == r.cur and r.n_matched == 0 and r.n_eligible == c.cfg.n_services
            assert r.spans_base == r.spans_cur > 0
        for a, b in ((c.base - 1, c.base), (c.base, c.base + 16)):  # one window outside the ring
            _raises(_lib.SA_ERANGE, lambda: e.window_latency_movers((a, b), (c.base, c.base)))
            _raises(_lib.SA_ERANGE, lambda: e.window_latency_movers((c.base, c.base), (a, b)))
        _check_calls(e, c, c.calls[:1])


def test_long_ranges():
    c = mu.case("long")
    assert all((h.sum(axis=1) > 0).all() for h in c.ref.values()) and len(c.ref) == 256  # every row a stripe reads counts
    with mu.loaded(c) as e:
        rs = _check_calls(e, c)
        assert [r.cur[1] - r.cur[0] + 1 for r in rs[::2]] == list(mu.LONG_LENGTHS)
        assert rs[-1].n_matched == 0 and rs[-2].n_matched == 0 and rs[-1].spans_cur == rs[-1].spans_base  # 256: equal ranges
        assert sum(r.n_matched for r in rs) >= 10


def test_select_path():
    c = mu.case("select")
    with mu.loaded(c) as e:
        full, one, ten = _check_calls(e, c)
        assert full.n_matched > mu.SELECT_K == len(full.services)
        w = mu.want(c, c.calls[0])
        k = mu.SELECT_K
        assert (w.order_shift[k - 1], w.order_count[k - 1]) == (w.order_shift[k], w.order_count[k])  # a class straddles the cut
        assert 0 in full.services  # key 0 goes through the select and the sort like any other
        assert one.services.tolist() == full.services[:1].tolist() and ten.services.tolist() == full.services[:10].tolist()
        mu.same(full, mu.run(e, c.calls[0]))


def test_at_the_bound():
    b = mu.bound_case()
    with Engine(b.cfg) as e:
        e.window_advance(b.w0)
        e.ingest(b.batch)
        r = e.window_latency_movers(b.B, b.C, mu.SELECT_K, mu.Q3)
        mu.assert_latency_movers(r, b.want, "bound")
        assert r.n_services == mu.BOUND_S and r.n_matched >= 20 and len(b.ids) >= 200
        last = e.window_latency(b.B[0], b.C[1], services=[0, mu.BOUND_S - 1], quantiles=mu.Q3)
        assert (last.count[0] > 0).all()  # the first and the last id have spans


@functools.lru_cache(maxsize=1)
def scratch_case():
    """A table of 8,192 slots with more than 4,096 ERROR series (window_top's
    select has work) and 10,000 services (so has the latency movers')."""
    cfg = Config(key_capacity=6000, bounds=(1, 10, 100), hll_p=4, n_services=10_000, n_windows=2,
                 options=OPT_WINDOW_LATENCY)
    w0 = ring_start(cfg)
    batch = make_batch(np.random.default_rng(zlib.crc32(b"latmov_scratch")), 120_000, cfg, 5600, w0=w0,
                       distinct_traces=True)
    extra = mu.drawn(zlib.crc32(b"latmov_scratch2"), cfg, w0, 60_000)
    extra = SpanBatch(np.zeros(len(extra), np.uint64), *extra.columns()[1:])  # key 0: the latency ring only
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(in_ring(batch, cfg, w0))
    cms = top_util.cells({w: o.window(w) for w in (w0, w0 + 1)}, w0, w0 + 1)
    steps = [(w0, batch), (w0, extra)]
    return SimpleNamespace(name="scratch", cfg=cfg, steps=steps, base=w0, cms=cms, cand=top_util.candidates([batch]),
                           ref=lu.window_hists(cfg, steps))


def test_scratch_shared_with_window_top():
    c = scratch_case()
    w0 = c.base
    call = ((w0, w0), (w0 + 1, w0 + 1), mu.SELECT_K, mu.PPM3, 1, 1, False)
    top_want, mov_want = top_util.top(c.cms, c.cand, top_util.TOP_MAX_K), mu.want(c, call)
    assert top_want.n_matched > top_util.TOP_MAX_K and mov_want.n_matched > mu.SELECT_K
    with mu.loaded(c) as e:
        assert e.stats()["table_capacity"] == 8192 < c.cfg.n_services  # fewer slots than candidates
        got = []
        for _ in range(2):
            top_util.assert_top_equal(e.window_top(w0, w0 + 1, top_util.TOP_MAX_K), top_want, "top")
            got.append(mu.run(e, call))
            mu.assert_latency_movers(got[-1], mov_want, "movers")
        mu.same(got[0], got[1])


def test_binned_engine():
    c = mu.case("services257")
    cfg = dataclasses.replace(c.cfg, key_capacity=300_000)
    with mu.loaded(c, cfg=cfg) as e:
        g = e.debug_geometry()
        assert g["path"] == "Binned" and e.stats()["table_capacity"] == 1 << 19
        _check_calls(e, c)


def test_call_behind_an_unsynchronised_device_ingest():
    c = mu.case("services64")
    (base, batch), = c.steps
    with Engine(c.cfg) as e:
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_latency_movers"))
        feed("F")  # on a stream of its own; nothing waits for it
        rs = _check_calls(e, c)
        assert rs[0].spans_base + rs[0].spans_cur == len(batch)  # the call joined the launch itself
        mu.same(rs[0], mu.run(e, c.calls[0]))


@pytest.mark.parametrize("option", [OPT_GROUP_COPY, OPT_GROUP_RCCL])
def test_group_equals_one_engine(option):
    """Three members on device 0 (a communicator cannot hold two of them: such
    a group merges through device copies whatever it asks for)."""
    gcfg = lambda c: dataclasses.replace(c.cfg, options=c.cfg.options | option)
    for name in ("ranges", "services257"):
        c = mu.case(name)
        with mu.loaded(c, Group, [0, 0, 0], cfg=gcfg(c)) as g, mu.loaded(c) as e:
            assert g.size == 3
            members = [int(g.lib.sa_group_member(g._h, i)) for i in range(3)]
            assert len(set(members)) == 3
            for call in c.calls:
                rg = mu.run(g, call)
                mu.assert_latency_movers(rg, mu.want(c, call), (name, call[2:]))
                mu.same(rg, mu.run(e, call))
            _raises(_lib.SA_ERANGE, lambda: g.window_latency_movers((c.base - 1, c.base), (c.base, c.base)))
            _raises(_lib.SA_EINVAL, lambda: g.window_latency_movers((c.base, c.base), (c.base, c.base), k=0))
            mu.same(mu.run(g, c.calls[0]), mu.run(e, c.calls[0]))
    c = mu.case("ranges")
    with Group([0, 0], dataclasses.replace(c.cfg, options=option)) as g:  # without the option
        _raises(_lib.SA_ESTATE, lambda: g.window_latency_movers((c.base, c.base), (c.base, c.base)))


def test_errors_leave_the_engine_usable():
    c = mu.case("ranges")
    b, W = c.base, c.cfg.n_windows
    call0 = c.calls[0]
    with mu.loaded(c) as e:
        ok = lambda: mu.assert_latency_movers(mu.run(e, call0), mu.want(c, call0), "after an error")
        out = C.POINTER(_lib.sa_latency_movers_result)()
        ppm, nine = (C.c_uint32 * 3)(*mu.PPM3), (C.c_uint32 * 9)(*([500_000] * 9))
        zero, big = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1_000_001)
        B, Cr = (b, b + 3), (b + 4, b + 7)

        def raw(k=10, q=ppm, nq=3, flags=0, o=out, base=B, cur=Cr):
            return e.lib.sa_window_latency_movers(e._h, base[0], base[1], cur[0], cur[1], k, 1, 1, q, nq, flags,
                                                  C.byref(o) if o is not None else None)

        bad = [dict(k=0), dict(k=_lib.SA_TOP_MAX_K + 1), dict(nq=0), dict(q=nine, nq=9), dict(q=None),
               dict(q=zero, nq=1), dict(q=big, nq=1), dict(flags=2), dict(flags=3)]
        for kw in bad:
            assert raw(**kw) == _lib.SA_EINVAL and not out, kw
            ok()
        assert raw(o=None) == _lib.SA_EINVAL  # a null `out`
        ok()
        for rng_ in ((b + 1, b), (b - 1, b), (b, b + W), (b + W, b + W), (0, 0)):
            assert raw(base=rng_) == _lib.SA_ERANGE and not out, rng_
            assert raw(cur=rng_) == _lib.SA_ERANGE and not out, rng_
            ok()
        assert raw(k=_lib.SA_TOP_MAX_K, q=nine, nq=8, flags=_lib.SA_LATMOV_FALL) == _lib.SA_OK and out
        assert out.contents.n_q == 8 and out.contents.flags == 1 and out.contents.n_services == c.cfg.n_services
        e.lib.sa_latency_movers_result_free(out)
    with Engine(dataclasses.replace(c.cfg, options=0)) as e:  # without the option
        e.window_advance(b)
        _raises(_lib.SA_ESTATE, lambda: e.window_latency_movers((b, b), (b, b)))
        assert e.stats()["window_base"] == b
