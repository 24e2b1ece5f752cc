"""sa_window_latency_onset on the GPU (spanagg_latency.hip's onset_thr_kernel,
onset_scan_kernel and onset_rows_kernel behind the movers' sums kernel and the
SLO's pairs kernel) against the numpy restatement of tests/onset_util.py, whose
workloads these are; every comparison is ==.

  range length          1 window (no split), 2, 64 and 65 (the scan's carry
                        across one step), 127 and 128, on a 128-window ring of 3
                        services
  moved ring            32 windows moved by 13 (the slots wrap): both
                        thresholds, rise and fall
  service counts        1, 64, 129 and 1,000 services on 8 windows, k of 1, 10
                        and SA_TOP_MAX_K: the gather, the grid, n_matched > k
  every threshold bin   256 services cut at bin s each (given), and every
                        service cut at bin b (pooled) for b at every lane boundary
  the crafted case, the 128-bit arithmetic and a 200-window random case through
  sa_onset_probe, consistency with sa_window_slo on the same engine, equal
  bits, a query behind an unsynchronised device ingest, every error return,
  groups of three and of one member over both transports.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import onset_util as ou
from ring_util import DeviceFeed
from spanagg import TOP_MAX_K, Config, Engine, Group, SpanAggError, _lib
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
    c = ou.case(name)
    with _loaded(c) as e:
        for j, call in enumerate(c.calls):
            ou.assert_onset(e.window_latency_onset(*call.args()), ou.want(name, j), (name, j))


def test_range_lengths():
    _check_case("lengths")
    lengths = sorted({call.last - call.first + 1 for call in ou.case("lengths").calls})
    assert lengths == [1, 2, 64, 65, 127, 128] and ou.want("lengths", 0).n_eligible == 0


def test_moved_ring():
    _check_case("moved")
    calls = ou.case("moved").calls
    assert {(call.thresholds is None, call.fall) for call in calls} == {(True, False), (False, False), (True, True),
                                                                        (False, True)}


@pytest.mark.parametrize("S", [1, 64, 129, 1000])
def test_service_counts(S):
    _check_case(f"services{S}")
    assert [call.k for call in ou.case(f"services{S}").calls][:3] == [1, 10, TOP_MAX_K]


def test_every_threshold_bin():
    _check_case("every_bin")
    w = ou.want("every_bin", 0)  # (what the restatement gives is what the workload's text states)
    assert w.threshold_bin.tolist() == list(range(255)) and w.slow_after.tolist() == [255 - s for s in range(255)]
    assert set(ou.want("every_bin", 5).threshold_bin.tolist()) == {ou.EVERY_BIN_POOLED[4]}


def test_crafted_case_step_by_step():
    c = ou.case("crafted")
    with _loaded(c) as e:
        rise = e.window_latency_onset(*c.calls[0].args())
        ou.assert_onset(rise, ou.want("crafted", 0))
        assert rise.items() == [(0, c.w0 + 3, 445_000, 200, 1, 300, 135)]  # the tie with w0 + 2 goes to the later split
        assert (rise.n_services, rise.n_eligible, rise.n_matched, rise.spans) == (1, 1, 1, 500)
        assert rise.threshold_bin.tolist() == [100] and rise.effective_ns.tolist() == [ou.su.CRAFTED_THRESHOLD]
        at200 = e.window_latency_onset(*c.calls[1].args())
        assert at200.items() == rise.items() and at200.min_count == 200
        at201 = e.window_latency_onset(*c.calls[2].args())
        assert (at201.n_eligible, at201.n_matched, at201.items()) == (0, 0, [])
        fall = e.window_latency_onset(*c.calls[3].args())  # the best D is -8,900: eligible, not matched
        assert (fall.n_eligible, fall.n_matched, fall.items(), fall.fall) == (1, 0, [], True)
        for j in range(4, len(c.calls)):
            ou.assert_onset(e.window_latency_onset(*c.calls[j].args()), ou.want("crafted", j), j)
    c = ou.case("crafted_rev")
    with _loaded(c) as e:
        rev = e.window_latency_onset(*c.calls[3].args())
        assert rev.items() == [(0, c.w0 + 4, 445_000, 300, 135, 200, 1)]
        for j, call in enumerate(c.calls):
            ou.assert_onset(e.window_latency_onset(*call.args()), ou.want("crafted_rev", j), j)
    c = ou.case("crafted_flat")
    with _loaded(c) as e:
        flat = e.window_latency_onset(*c.calls[0].args())  # D == 0 everywhere: eligible, not matched
        assert (flat.n_eligible, flat.n_matched, flat.spans, flat.items()) == (1, 0, 60, [])
        for j, call in enumerate(c.calls):
            ou.assert_onset(e.window_latency_onset(*call.args()), ou.want("crafted_flat", j), j)


@pytest.mark.parametrize("name", ou.PROBES)
def test_probe_on_given_pairs(name):
    """big: counts near 2^43, products past 2^86 -- the restatement that wraps D
    to 64 bits picks other splits and another order (the host tests show it);
    random200: four steps of the scan; ties: the hand-made rows."""
    c = ou.probe(name)
    with Engine(Config(n_services=1, n_windows=4, hll_p=10, key_capacity=1000)) as e:  # (any engine: no ring is read)
        for j, call in enumerate(c.calls):
            ou.assert_onset(e.onset_probe(c.pairs, *call.args()), ou.want_probe(name, j), (name, j))
        if name == "big":
            wrong = ou.expected_probe(c.pairs, *c.calls[0].args(), wrong="d_i64")
            got = e.onset_probe(c.pairs, *c.calls[0].args())
            assert got.services.tolist() != wrong.services.tolist()
            assert got.onset_window.tolist() == ou.want_probe(name, 0).splits
        out = C.POINTER(_lib.sa_onset_result)()
        p = np.zeros((2, 3, 2), np.uint64)
        raw = lambda n_sel=2, n_cov=3, k=1, flags=0, ptr=p.ctypes.data_as(_lib.u64p): e.lib.sa_onset_probe(
            e._h, ptr, n_sel, n_cov, k, 1, 1, flags, C.byref(out))
        for kw in (dict(n_sel=0), dict(n_cov=0), dict(k=0), dict(k=TOP_MAX_K + 1), dict(flags=2), dict(ptr=None),
                   dict(n_sel=1 << 10, n_cov=(1 << 8) + 1)):
            assert raw(**kw) == _lib.SA_EINVAL and not out, kw
        ou.assert_onset(e.onset_probe(c.pairs, *c.calls[0].args()), ou.want_probe(name, 0))


def test_consistent_with_window_slo_on_the_same_engine():
    c = ou.case("moved")
    with _loaded(c) as e:
        rows = 0
        for call in c.calls:
            r = e.window_latency_onset(*call.args())
            for i, s in enumerate(r.services.tolist()):
                onset, thr = int(r.onset_window[i]), [int(r.effective_ns[i])]
                before = e.window_slo(onset - 1, onset - 1, (onset - call.first,), (0,), thr, [s])
                after = e.window_slo(call.last, call.last, (call.last - onset + 1,), (0,), thr, [s])
                assert (int(before.total[0, 0, 0]), int(before.slow[0, 0, 0])) == (int(r.total_before[i]), int(r.slow_before[i]))
                assert (int(after.total[0, 0, 0]), int(after.slow[0, 0, 0])) == (int(r.total_after[i]), int(r.slow_after[i]))
                assert int(before.threshold_bin[0]) == int(r.threshold_bin[i])
                rows += 1
        assert rows >= 2
    c = ou.case("services129")
    with _loaded(c) as e:
        call = c.calls[1]
        r = e.window_latency_onset(*call.args())
        assert len(r.services) == 10
        onsets = sorted(set(r.onset_window.tolist()))
        for onset in onsets:  # one sa_window_slo call an onset window, every returned service of it
            m = np.flatnonzero(r.onset_window == onset)
            sv, thr = r.services[m].tolist(), r.effective_ns[m].tolist()
            before = e.window_slo(onset - 1, onset - 1, (onset - call.first,), (0,), thr, sv)
            after = e.window_slo(call.last, call.last, (call.last - onset + 1,), (0,), thr, sv)
            assert np.array_equal(before.total[0, 0], r.total_before[m]) and np.array_equal(before.slow[0, 0], r.slow_before[m])
            assert np.array_equal(after.total[0, 0], r.total_after[m]) and np.array_equal(after.slow[0, 0], r.slow_after[m])


def test_two_calls_give_equal_bits():
    c = ou.case("lengths")
    with _loaded(c) as e:
        a = e.window_latency_onset(*c.calls[10].args())
        other = e.window_latency_onset(*c.calls[3].args())  # (another shape and mode in between: the scratch is reused)
        ou.assert_onset(other, ou.want("lengths", 3))
        e.onset_probe(ou.probe("ties").pairs, 3)            # ... and the probe's, of other services
        ou.same(e.window_latency_onset(*c.calls[10].args()), a)
        ou.assert_onset(a, ou.want("lengths", 10))


def test_query_behind_an_unsynchronised_device_ingest():
    c = ou.case("moved")
    (b0, first_batch), (base, batch) = c.steps
    with Engine(c.cfg) as e:
        e.window_advance(b0)
        e.ingest(first_batch)
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_onset"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_latency_onset(*c.calls[0].args())
        ou.assert_onset(r, ou.want("moved", 0))
        ou.same(e.window_latency_onset(*c.calls[0].args()), r)


def test_errors_leave_the_engine_usable():
    c = ou.case("services64")
    call, W, S = c.calls[1], c.cfg.n_windows, c.cfg.n_services
    first, last = c.w0, c.w0 + W - 1
    with _loaded(c) as e:
        ok = lambda: ou.assert_onset(e.window_latency_onset(*call.args()), ou.want("services64", 1))
        out = C.POINTER(_lib.sa_onset_result)()
        thr = (C.c_uint64 * S)(*([1000] * S))

        def raw(k=1, q_ppm=500_000, thresholds=None, flags=0, o=out, a=first, b=last):
            return e.lib.sa_window_latency_onset(e._h, a, b, k, q_ppm, thresholds, 1, 1, flags,
                                                 C.byref(o) if o is not None else None)

        bad = [dict(k=0), dict(k=TOP_MAX_K + 1),                       # k outside 1..SA_TOP_MAX_K
               dict(flags=2), dict(flags=3),                           # flag bits other than SA_ONSET_FALL
               dict(q_ppm=0), dict(q_ppm=1_000_001),                   # pooled: q_ppm outside 1..10^6
               dict(thresholds=thr), dict(thresholds=thr, q_ppm=1)]    # given: q_ppm must be 0
        for kw in bad:
            assert raw(**kw) == _lib.SA_EINVAL and not out, kw
            ok()
        assert raw(o=None) == _lib.SA_EINVAL  # a null `out`
        for a, b in ((first + 1, first), (first - 1, last), (first, last + 1), (0, 0), (last + 1, last + 1)):
            _raises(_lib.SA_ERANGE, lambda: e.window_latency_onset(a, b))
            ok()
        assert raw(thresholds=thr, q_ppm=0, k=TOP_MAX_K, flags=1) == _lib.SA_OK and out
        assert (out.contents.k, out.contents.flags, out.contents.q_ppm, out.contents.n_services) == (TOP_MAX_K, 1, 0, S)
        e.lib.sa_onset_result_free(out)
        with pytest.raises(ValueError):  # (the wrapper: one threshold a service)
            e.window_latency_onset(first, last, thresholds_ns=[1000] * (S - 1))
        r = e.window_latency_onset(first, last, min_delta_ppm=1_000_001)  # matches nothing
        assert (r.n_matched, len(r.services)) == (0, 0) and r.n_eligible > 0
        assert e.window_latency_onset(first, last, min_count=0).min_count == 1  # (min_count 0 is applied as 1)
        ok()
    with Engine(dataclasses.replace(c.cfg, options=0)) as e:  # without the option
        e.window_advance(c.w0)
        _raises(_lib.SA_ESTATE, lambda: e.window_latency_onset(*call.args()))
        assert e.stats()["window_base"] == c.w0


@pytest.mark.parametrize("devices,option,rccl", [([0, 0, 0], OPT_GROUP_COPY, False), ([0, 0, 0], OPT_GROUP_RCCL, False),
                                                 ([0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True)])
def test_group_equals_one_engine(devices, option, rccl):
    """Members on device 0 (a communicator cannot hold two of them: those
    groups merge through device copies whatever they ask for); a group of one
    that asks for RCCL all-reduces for real.  Both threshold modes: the pooled
    one takes two rounds of the transport."""
    for name in ("moved", "services129"):
        c = ou.case(name)
        gcfg = dataclasses.replace(c.cfg, options=c.cfg.options | option)
        with _loaded(SimpleNamespace(cfg=gcfg, steps=c.steps), Group, devices) as g, _loaded(c) as e:
            assert g.size == len(devices) and g.uses_rccl == rccl
            assert {call.thresholds is None for call in c.calls} == {True, False}
            for j, call in enumerate(c.calls):
                rg = g.window_latency_onset(*call.args())
                ou.assert_onset(rg, ou.want(name, j), (name, j))
                ou.same(rg, e.window_latency_onset(*call.args()), (name, j))
            call = c.calls[0]
            _raises(_lib.SA_ERANGE, lambda: g.window_latency_onset(call.last + 1, call.last + 1))
            _raises(_lib.SA_ERANGE, lambda: g.window_latency_onset(call.last, call.first - 1))
            _raises(_lib.SA_EINVAL, lambda: g.window_latency_onset(call.first, call.last, 0))
            _raises(_lib.SA_EINVAL, lambda: g.window_latency_onset(call.first, call.last, quantile=0.0))
            ou.same(g.window_latency_onset(*call.args()), e.window_latency_onset(*call.args()), name)
    with Group([0, 0], dataclasses.replace(gcfg, options=option)) as g:  # without the option
        _raises(_lib.SA_ESTATE, lambda: g.window_latency_onset(*call.args()))
