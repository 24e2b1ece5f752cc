"""sa_window_slo on the GPU (spanagg_latency.hip's slo_pairs_kernel and
slo_slide_kernel) against the numpy restatement of tests/slo_util.py, whose
workloads these are; every comparison is ==.

  every threshold bin   256 services, one span in each of the 256 bins, service
                        s's threshold at bin s: the lane mask at every lane
                        boundary and the open last bin
  service counts        1, 64, 129 and 1,000 services, every one selected
  moved ring            32 windows moved by 13 (the slots wrap): widths (1, 2,
                        5) over 28 outputs, widths (31, 32) at one
  long scan             128 and 127 covered windows: the carry across 64-window
                        chunks, a last chunk that is not full
  an unsorted selection, consistency with sa_window_latency on the same engine,
  the crafted burn edges, idempotence, a query behind an unsynchronised device
  ingest, every error return, groups of three and of one member over both
  transports.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import slo_util as su
from ring_util import DeviceFeed
from spanagg import SLO_MAX_WIDTHS, Engine, Group, SpanAggError, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

pytestmark = pytest.mark.gpu


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def _loaded(c, cls=Engine, *a):
    x = cls(*a, c.cfg) if a else cls(c.cfg)
    for base, batch in c.steps:
        x.window_advance(base)
        x.ingest(batch)
    return x


def _check_case(name):
    c = su.case(name)
    with _loaded(c) as e:
        for j, call in enumerate(c.calls):
            su.assert_slo(e.window_slo(*call.args()), su.want(name, j), (name, j))


def test_every_threshold_bin():
    _check_case("every_bin")
    w = su.want("every_bin", 0)  # (what the restatement gives is what the issue states)
    assert w.total[0, 0].tolist() == [256] * 256 and w.slow[0, 0].tolist() == [255 - s for s in range(256)]


@pytest.mark.parametrize("S", [1, 64, 129, 1000])
def test_service_counts(S):
    _check_case(f"services{S}")


def test_moved_ring():
    _check_case("moved")


def test_long_scan():
    _check_case("long")


def test_selection_is_echoed_in_the_callers_order():
    c = su.case("selection")
    with _loaded(c) as e:
        for j, call in enumerate(c.calls):
            r = e.window_slo(*call.args())
            su.assert_slo(r, su.want("selection", j), j)
            assert r.services.tolist() == list(call.services) and r.threshold_ns.tolist() == list(call.thresholds)
            assert r.widths.tolist() == list(call.widths) and r.limit_ppm.tolist() == list(call.limit_ppm)
        assert e.window_slo(*c.calls[1].args()).min_count == 1  # (min_count 0 is applied as 1)
        assert len(c.calls[1].widths) == SLO_MAX_WIDTHS


def test_consistent_with_window_latency_on_the_same_engine():
    c = su.case("moved")
    with _loaded(c) as e:
        for call in c.calls:
            r = e.window_slo(*call.args())
            for i, s in enumerate(r.services.tolist()):
                tb = int(r.threshold_bin[i])
                for w, width in enumerate(call.widths):
                    for o, t in enumerate(range(call.first, call.last + 1)):
                        one = e.window_latency_series(t, t, width, services=[s], hist=True)
                        assert int(r.total[o, w, i]) == int(one.count[0, 0]), (t, width, s)
                        assert int(r.slow[o, w, i]) == int(one.hist[0, 0, tb + 1:].sum(dtype=np.uint64)), (t, width, s)


def test_crafted_burn_edges():
    c = su.crafted()
    with Engine(c.cfg) as e:
        e.window_advance(c.w0)
        fed = 0
        for j, (n, call, bits, alerts) in enumerate(c.calls):
            for _, batch in c.steps[fed:n]:
                e.ingest(batch)
            fed = max(fed, n)
            r = e.window_slo(*call.args())
            su.assert_slo(r, su.expected(c.refs[n], c.cfg, call), j)
            assert r.burning[:, 0].tolist() == bits and r.alert_outputs.tolist() == [alerts], j
        first = e.window_slo(*c.calls[7][1].args())  # after the 11th slow span
        assert (int(first.total[0, 0, 0]), int(first.slow[0, 0, 0])) == (1001, 11)


def test_two_calls_give_equal_bits():
    c = su.case("long")
    with _loaded(c) as e:
        a = e.window_slo(*c.calls[0].args())
        other = e.window_slo(*c.calls[1].args())  # (another shape in between: the scratch is reused)
        su.assert_slo(other, su.want("long", 1))
        su.same(e.window_slo(*c.calls[0].args()), a)


def test_query_behind_an_unsynchronised_device_ingest():
    c = su.case("moved")
    (b0, first_batch), (base, batch) = c.steps
    with Engine(c.cfg) as e:
        e.window_advance(b0)
        e.ingest(first_batch)
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_slo"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_slo(*c.calls[0].args())
        su.assert_slo(r, su.want("moved", 0))
        su.same(e.window_slo(*c.calls[0].args()), r)


def test_errors_leave_the_engine_usable():
    c = su.case("selection")
    call, W, S = c.calls[0], c.cfg.n_windows, c.cfg.n_services
    first, last = c.w0, c.w0 + W - 1
    with _loaded(c) as e:
        ok = lambda: su.assert_slo(e.window_slo(*call.args()), su.want("selection", 0))
        out = C.POINTER(_lib.sa_slo_result)()
        u32 = lambda *v: (C.c_uint32 * len(v))(*v)
        thr = (C.c_uint64 * S)(*([1000] * S))
        w1, lim, five = u32(1), u32(1000), u32(1, 1, 1, 1, 1)

        def raw(widths=w1, limits=lim, n_widths=1, services=None, n_sel=0, thresholds=thr, flags=0, o=out, a=last, b=last):
            return e.lib.sa_window_slo(e._h, a, b, widths, limits, n_widths, services, n_sel, thresholds, 1, flags,
                                       C.byref(o) if o is not None else None)

        bad = [dict(n_widths=0), dict(widths=five, limits=five, n_widths=5),   # n_widths outside 1..4
               dict(widths=None), dict(limits=None),                           # null widths, null limit_ppm
               dict(limits=u32(1_000_001)),                                    # a limit above 10^6
               dict(thresholds=None),                                          # null threshold_ns
               dict(flags=1),                                                  # flags are reserved
               dict(services=None, n_sel=1), dict(services=u32(0), n_sel=0),   # services == NULL with n_sel != 0, the reverse
               dict(services=u32(0, S), n_sel=2), dict(services=u32(3, 3), n_sel=2)]  # an id >= n_services, a repeat
        for kw in bad:
            assert raw(**kw) == _lib.SA_EINVAL and not out, kw
            ok()
        assert raw(o=None) == _lib.SA_EINVAL  # a null `out`
        one = lambda a, b, widths: e.window_slo(a, b, widths, [1000] * len(widths), [1000] * S)
        for a, b, widths in ((first + 1, first, (1,)), (first, last, (0,)), (last, last, (1, W + 1)), (first, last, (1, 2)),
                             (first, last, (2, 1)), (first - 1, last, (1,)), (first, last + 1, (1,)), (0, 0, (2,))):
            _raises(_lib.SA_ERANGE, lambda: one(a, b, widths))
            ok()
        assert raw(widths=u32(W), a=last, b=last) == _lib.SA_OK and out and out.contents.n_sel == S
        assert out.contents.n_out == 1 and out.contents.n_widths == 1
        e.lib.sa_slo_result_free(out)
        with pytest.raises(ValueError):  # (the wrapper: one threshold a selected service)
            e.window_slo(last, last, (1,), (1000,), [1000] * (S - 1))
        ok()
    with Engine(dataclasses.replace(c.cfg, options=0)) as e:  # without the option
        e.window_advance(c.w0)
        _raises(_lib.SA_ESTATE, lambda: e.window_slo(*call.args()))
        assert e.stats()["window_base"] == c.w0


def test_every_row_of_the_largest_ring():
    """n_out * n_sel > 2^20 cannot be met while sa_create holds the ring to 2^18
    rows: every output and service of the largest ring is a good call."""
    from spanagg import Config
    from geometry_util import ring_start
    cfg = Config(n_services=4096, n_windows=64, hll_p=4, key_capacity=1000, options=_lib.OPT_WINDOW_LATENCY)
    w0 = ring_start(cfg)
    with Engine(cfg) as e:
        e.window_advance(w0)
        r = e.window_slo(w0, w0 + 63, (1,), (0,), [0] * 4096)
        assert r.total.shape == (64, 1, 4096) and not r.total.any() and not r.burning.any() and not r.alert_outputs.any()


@pytest.mark.parametrize("devices,option,rccl", [([0, 0, 0], OPT_GROUP_COPY, False), ([0, 0, 0], OPT_GROUP_RCCL, False),
                                                 ([0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True)])
def test_group_equals_one_engine(devices, option, rccl):
    """Members on device 0 (a communicator cannot hold two of them: those
    groups merge through device copies whatever they ask for); a group of one
    that asks for RCCL all-reduces for real."""
    for name in ("moved", "selection"):
        c = su.case(name)
        gcfg = dataclasses.replace(c.cfg, options=c.cfg.options | option)
        with _loaded(SimpleNamespace(cfg=gcfg, steps=c.steps), Group, devices) as g, _loaded(c) as e:
            assert g.size == len(devices) and g.uses_rccl == rccl
            for j, call in enumerate(c.calls):
                rg = g.window_slo(*call.args())
                su.assert_slo(rg, su.want(name, j), (name, j))
                su.same(rg, e.window_slo(*call.args()), (name, j))
            call = c.calls[0]
            S = len(call.thresholds)
            _raises(_lib.SA_ERANGE, lambda: g.window_slo(call.first, call.last, (c.cfg.n_windows + 1,), (0,), call.thresholds,
                                                         call.services))
            _raises(_lib.SA_ERANGE, lambda: g.window_slo(call.last + 1, call.last + 1, (1,), (0,), call.thresholds,
                                                         call.services))
            _raises(_lib.SA_EINVAL, lambda: g.window_slo(call.first, call.last, (1,), (1_000_001,), call.thresholds,
                                                         call.services))
            _raises(_lib.SA_EINVAL, lambda: g.window_slo(call.first, call.last, (1,) * 5, (0,) * 5, call.thresholds,
                                                         call.services))
            _raises(_lib.SA_EINVAL, lambda: g.window_slo(call.first, call.last, (1,), (0,), [0] * S, (0,) * S if S > 1
                                                         else (c.cfg.n_services,)))
            su.same(g.window_slo(*call.args()), e.window_slo(*call.args()), name)
    with Group([0, 0], dataclasses.replace(gcfg, options=option)) as g:  # without the option
        _raises(_lib.SA_ESTATE, lambda: g.window_slo(*call.args()))
