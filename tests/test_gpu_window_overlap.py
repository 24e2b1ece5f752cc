"""Service overlap over the window ring (sa_window_overlap,
sa_group_window_overlap) against the CPU oracle: per selected service the
merged registers' histogram, per pair the histogram of the register-wise
maximum -- every comparison with == (tests/overlap_util.py builds the cases
and the references; tests/test_window_overlap_host.py proves the inputs can
catch a wrong pair index, a missing maximum, pairing per window and a range
short of a window).

  * hll_p 4 (a service is one thread's 16-byte load, the tile mostly empty),
    hll_p 18 (one pair, a bin past 65,535, many chunks), hll_p 8 with 64
    services (full and diagonal tiles, every one of the 2,016 pairs);
  * the default hll_p with 200 services: selections of 5 and 9 ids, unsorted
    and non-contiguous (the service map, ragged tiles, the caller's order),
    and services=None refused;
  * selections of one and of two;
  * every sub-range of a moved ring;
  * a binned and a dense-index engine, and a device ingest nothing waited for;
  * idempotence, and nothing cleared: window_range, window_read and flush
    answer as the oracle afterwards;
  * groups of two and three members over both transports;
  * every error return, each followed by a good call.

Every result is also checked for rows summing to 2^p, for hist / distinct
equal to window_range's rows, and for union / shared / strongest equal to the
arithmetic on the returned histograms (overlap_util.assert_overlap_equal).
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import overlap_util as ou
import pyoracle
from geometry_util import assert_geometry
from overlap_util import assert_overlap_equal, case, expected, reference
from parity_util import assert_red_equal
from ring_util import DeviceFeed
from spanagg import OVERLAP_MAX_SERVICES, Config, Engine, Group, SpanAggError, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL

pytestmark = pytest.mark.gpu


def _loaded(name):
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
    return e, c


def _check(x, c, first, last, services=None, ranged=None):
    """x.window_overlap(first, last, services) against the oracle, and its
    hist / distinct against x.window_range's rows (ranged: a RangeResult of
    the same range already at hand)."""
    ids = list(range(c.cfg.n_services)) if services is None else list(services)
    want = expected(reference(c.name), range(first, last + 1), ids, c.cfg.hll_p)
    r = x.window_overlap(first, last, services)
    assert (r.first, r.last) == (first, last)
    assert_overlap_equal(r, want, c.cfg, (c.name, first, last, services))
    rr = ranged or x.window_range(first, last)
    assert np.array_equal(r.hist, rr.hist[ids]) and np.array_equal(r.distinct, rr.distinct[ids])
    return r


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def test_p4_one_word_a_service():
    e, c = _loaded("p4")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, first, last)
        assert r.pair_hist.shape == (3, 64) and r.hist.sum() == 3 * 16
        _check(e, c, first, first, (2, 0))


def test_p18_one_pair_and_a_bin_past_16_bits():
    e, c = _loaded("p18")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, first, last)
        assert r.pair_hist.shape == (1, 64) and r.pair_hist.max() > 65535
        assert 0.45 < r.shared[0, 1] / r.union[0, 1] < 0.55  # half the traces are on both


def test_every_pair_of_64_services():
    e, c = _loaded("p8x64")
    with e:
        (first, last), = c.ranges
        assert c.cfg.n_services == OVERLAP_MAX_SERVICES
        r = _check(e, c, first, last)
        assert len(r.pair_hist) == 2016
        a, b = ou.PLANT.SAME
        assert r.shared[a, b] == r.distinct[a] and r.shared[ou.PLANT.EMPTY, 9] == 0.0
        # the same pairs through another selection: reversed, so every pair index moves
        rev = list(range(63, -1, -1))
        q = _check(e, c, first, last, rev)
        assert np.array_equal(q.shared, r.shared[::-1, ::-1])
        # 63 and 57: a ragged last tile row, alone and beside full ones
        _check(e, c, first, last, range(1, 64))
        _check(e, c, first, last, range(3, 60))


def test_selections_of_200_services():
    e, c = _loaded("p14x200")
    with e:
        (first, last), = c.ranges
        rr = e.window_range(first, last)
        for sel in (ou.SEL5, ou.SEL9, ou.SEL9[::-1]):
            r = _check(e, c, first, last, sel, rr)
            assert list(r.services) == list(sel)
        a, b = ou.SEL5.index(ou.PLANT.SAME[0]), ou.SEL5.index(ou.PLANT.SAME[1])
        r = _check(e, c, first, last, ou.SEL5, rr)
        assert r.shared[a, b] == r.distinct[a] > 0 and r.shared[a, ou.SEL5.index(ou.PLANT.EMPTY)] == 0.0
        # more than SA_OVERLAP_MAX_SERVICES services: all of them cannot be asked for
        _raises(_lib.SA_EINVAL, lambda: e.window_overlap(first, last))
        _raises(_lib.SA_EINVAL, lambda: e.window_overlap(first, last, range(OVERLAP_MAX_SERVICES + 1)))
        _raises(_lib.SA_EINVAL, lambda: e.window_overlap(first, last, (1, 200)))
        # one and two
        one = _check(e, c, first, last, (121,), rr)
        assert one.pair_hist.shape == (0, 64) and one.shared.shape == (1, 1) and one.strongest(5) == []
        two = _check(e, c, first, last, (122, 121), rr)
        assert two.pair_hist.shape == (1, 64) and two.strongest(5) == [(122, 121, float(two.shared[0, 1]))]
        _check(e, c, first, last, range(100, 100 + OVERLAP_MAX_SERVICES), rr)


def test_sub_ranges_and_wrap_on_a_moved_ring():
    e, c = _loaded("moved")
    with e:
        assert len(c.ranges) == 10 and c.base & (c.cfg.n_windows - 1) != 0  # (the ring wraps inside)
        for first, last in c.ranges:
            _check(e, c, first, last)
            _check(e, c, first, last, (11, 4, 7))


@pytest.mark.parametrize("row", ou.ROWS)
def test_binned_and_dense_engines(row):
    e, c = _loaded(f"row:{row}")
    with e:
        (first, last), = c.ranges
        r = _check(e, c, first, last)
        assert r.shared[0, 1] > 0
        _check(e, c, first + 1, last - 1, (1, 0))


def test_idempotent_ordered_and_nothing_cleared():
    """Behind a device ingest nothing waited for; twice; then the other reads
    and the flush against the oracle."""
    c, windows = case("moved"), reference("moved")
    cfg = c.cfg
    (b0, first_batch), (base, batch) = c.steps
    W = cfg.n_windows
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o.ingest(first_batch)
    o.ingest(batch)
    with Engine(cfg) as e:
        e.window_advance(b0)
        e.ingest(first_batch)
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_overlap"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = _check(e, c, base, base + W - 1)
        again = e.window_overlap(base, base + W - 1)
        for f in ("services", "hist", "distinct", "pair_hist", "union", "shared"):
            assert np.array_equal(getattr(r, f), getattr(again, f)), f
        want = ou.merged(windows, range(base, base + W), ())
        rr = e.window_range(base, base + W - 1, registers=True, cells=True)
        assert np.array_equal(rr.hll, want.hll) and np.array_equal(rr.cms, want.cms)
        for w in range(base, base + W):
            sk = e.window_read(w)
            assert np.array_equal(sk.hll, windows[w][0]) and np.array_equal(sk.cms, windows[w][1]), w
        assert_red_equal(e.flush(), o.series(), unit_div=1e6)
        _check(e, c, base + 1, base + 2, (3, 9, 1))


@pytest.mark.parametrize("devices,option,rccl", [([0, 0], OPT_GROUP_COPY, False), ([0, 0, 0], OPT_GROUP_COPY, False),
                                                 ([0, 0], OPT_GROUP_RCCL, False), ([0, 0, 0], OPT_GROUP_RCCL, False)])
def test_group_equals_the_oracle_and_one_engine(devices, option, rccl):
    """Members on one device: a communicator cannot hold them, so a group that
    asks for RCCL merges through device copies too (as test_gpu_window_top's)."""
    c = case("moved")
    with Group(devices, dataclasses.replace(c.cfg, options=option)) as g, Engine(c.cfg) as e:
        assert g.size == len(devices) and g.uses_rccl == rccl
        for x in (g, e):
            for base, batch in c.steps:
                x.window_advance(base)
                x.ingest(batch)
        W = c.cfg.n_windows
        for first, last, sel in ((c.base, c.base + W - 1, None), (c.base + 1, c.base + 2, (10, 2, 1, 6, 5))):
            rg = _check(g, c, first, last, sel)
            re_ = e.window_overlap(first, last, sel)
            for f in ("services", "hist", "distinct", "pair_hist", "union", "shared"):
                assert np.array_equal(getattr(rg, f), getattr(re_, f)), f
        _raises(_lib.SA_ERANGE, lambda: g.window_overlap(c.base - 1, c.base))
        _raises(_lib.SA_EINVAL, lambda: g.window_overlap(c.base, c.base, (1, 1)))
        _raises(_lib.SA_EINVAL, lambda: g.window_overlap(c.base, c.base, (1, c.cfg.n_services)))
        _check(g, c, c.base, c.base, (0, 1))


def test_rccl_group_of_one():
    c = case("moved")
    with Group([0], dataclasses.replace(c.cfg, options=OPT_GROUP_RCCL)) as g:
        assert g.uses_rccl
        for base, batch in c.steps:
            g.window_advance(base)
            g.ingest(batch)
        _check(g, c, c.base, c.base + c.cfg.n_windows - 1)
        _check(g, c, c.base + 2, c.base + 3, (7, 8, 0))


def test_errors_leave_the_engine_usable():
    e, c = _loaded("moved")
    with e:
        first, last, W, S = c.base, c.base + c.cfg.n_windows - 1, c.cfg.n_windows, c.cfg.n_services
        out = C.POINTER(_lib.sa_overlap_result)()
        ids = (C.c_uint32 * 3)(2, 5, 2)
        call = lambda sv, n, flags, o=out: e.lib.sa_window_overlap(e._h, first, last, sv, n, flags,
                                                                   C.byref(o) if o is not None else None)
        bad = [(None, 2, 0), (ids, 3, 0), (ids, 2, 1), (ids, OVERLAP_MAX_SERVICES + 1, 0), (ids, 0, 0)]
        for sv, n, flags in bad:
            assert call(sv, n, flags) == _lib.SA_EINVAL and not out, (n, flags)
            _check(e, c, first, last, (2, 5))
        assert call(ids, 2, 0, None) == _lib.SA_EINVAL
        _raises(_lib.SA_EINVAL, lambda: e.window_overlap(first, last, (0, S)))
        _check(e, c, first, last, (0, S - 1))
        for a, b in ((first + 1, first), (first - 1, last), (first, first + W)):
            _raises(_lib.SA_ERANGE, lambda: e.window_overlap(a, b))
            _check(e, c, first, first)
        assert call(ids, 2, 0) == _lib.SA_OK and out and out.contents.n_pairs == 1
        e.lib.sa_overlap_result_free(out)
