"""Range queries over the window ring (sa_window_range, sa_group_window_range)
against the CPU oracle: HLL registers max-merged over the windows first..last,
their histogram per service, the count-min cells summed as u64 and point
queries on the sum -- all bit-exact (tests/range_util.py builds the cases and
the references; tests/test_window_range_host.py proves the inputs can catch a
wrong end of the range, a missing merge and a missing wrap).

  * every row of RING_ROWS (every ingest path): the whole ring as one range;
  * a moved ring (slots cleared and reused): every sub-range of ring_512, the
    ranges around the slot wrap of ring_1024_noerr; a range of one window
    equals window_read;
  * hll_p 4 (a service is one thread's 16-byte load) and 18 (a bin's count
    passes 65,535);
  * 0, 1 and 100,000 keys;
  * idempotence, ordering behind an unsynchronised device ingest, and the
    reads that follow;
  * the error returns;
  * groups over both transports, equal to the oracle and to one engine.
"""
import ctypes as C
import dataclasses
from types import SimpleNamespace

import numpy as np
import pytest

import range_util
from geometry_util import RING_ROWS, assert_geometry, check_against_oracle, key_pool
from range_util import assert_range_equal, case, merged, reference
from ring_util import DeviceFeed
from spanagg import Engine, Group, SpanAggError, _lib
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL
from spanagg.sketch import cms_query, heavy_hitters

pytestmark = pytest.mark.gpu


def _loaded(name):
    """A fresh engine of the case's config after the case's steps (host ingest)."""
    c = case(name)
    e = Engine(c.cfg)
    if c.row:
        assert_geometry(e, c.row)
    for base, batch in c.steps:
        e.window_advance(base)
        e.ingest(batch)
    return e, c


def _check_ranges(e, c):
    windows = reference(c.name)
    for first, last in c.ranges:
        r = e.window_range(first, last, c.keys, registers=True, cells=True)
        assert (r.first, r.last) == (first, last)
        want = merged(windows, range(first, last + 1), c.keys)
        assert_range_equal(r, want, c.cfg, (first, last))
        assert r.top_errors(10) == heavy_hitters(want.cms, c.keys, 10), (first, last)
        if first == last:  # one window: what window_read returns
            sk = e.window_read(first)
            assert np.array_equal(r.hll, sk.hll) and np.array_equal(r.cms, sk.cms), first


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_full_ring_on_every_path(row):
    e, c = _loaded(f"full:{row}")
    with e:
        _check_ranges(e, c)
        # the plain query: no registers, no cells, the same answers
        (first, last), = c.ranges
        plain = e.window_range(first, last, c.keys)
        want = merged(reference(c.name), range(first, last + 1), c.keys)
        assert plain.hll is None and plain.cms is None
        assert np.array_equal(plain.hist, want.hist) and np.array_equal(plain.errors, want.errors)


@pytest.mark.parametrize("row", range_util.MOVED)
def test_sub_ranges_and_wrap_on_a_moved_ring(row):
    e, c = _loaded(f"moved:{row}")
    with e:
        assert len(c.ranges) == (10 if row == "ring_512" else 6)
        _check_ranges(e, c)


@pytest.mark.parametrize("name", list(range_util.EXTREMES))
def test_extremes_of_hll_p(name):
    e, c = _loaded(name)
    with e:
        _check_ranges(e, c)


def test_key_counts():
    e, c = _loaded("full:ring_512")
    with e:
        (first, last), = c.ranges
        want = merged(reference(c.name), range(first, last + 1), c.keys[:1])
        none = e.window_range(first, last)
        assert none.errors.shape == (0,) and none.keys.shape == (0,) and none.top_errors() == []
        assert np.array_equal(none.hist, want.hist)
        one = e.window_range(first, last, c.keys[:1])
        assert np.array_equal(one.errors, want.errors) and want.errors[0] > 0
        rng = np.random.default_rng(100_000)
        many = np.concatenate([key_pool(RING_ROWS["ring_512"]["n_keys"]), np.zeros(1, np.uint64),
                               rng.integers(0, 2**64, 100_000, dtype=np.uint64)])[:100_000]
        r = e.window_range(first, last, many, cells=True)
        assert np.array_equal(r.cms, want.cms)
        assert [int(x) for x in r.errors] == [cms_query(want.cms, int(k)) for k in many]


def test_idempotent_and_ordered_behind_a_device_ingest():
    c, windows = case("full:ring_512"), reference("full:ring_512")
    (base, batch), = c.steps
    (first, last), = c.ranges
    want = merged(windows, range(first, last + 1), c.keys)
    with Engine(c.cfg) as e:
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_range"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_range(first, last, c.keys, registers=True, cells=True)
        assert_range_equal(r, want, c.cfg, "behind the ingest")
        again = e.window_range(first, last, c.keys, registers=True, cells=True)
        for f in ("hist", "distinct", "hll", "cms", "errors"):
            assert np.array_equal(getattr(r, f), getattr(again, f)), f
        check_against_oracle(e, [batch], c.cfg, base)  # flush and window_read after it


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def test_errors_leave_the_engine_usable():
    c = case("full:ring_512")
    (base, batch), = c.steps
    W = c.cfg.n_windows
    with Engine(c.cfg) as e:
        e.window_advance(base)
        e.ingest(batch)
        _raises(_lib.SA_ERANGE, lambda: e.window_range(base + 1, base))
        _raises(_lib.SA_ERANGE, lambda: e.window_range(base - 1, base + 1))
        _raises(_lib.SA_ERANGE, lambda: e.window_range(base, base + W))
        out = C.POINTER(_lib.sa_range_result)()
        key = (C.c_uint64 * 1)(5)
        assert e.lib.sa_window_range(e._h, base, base, None, 0, 4, C.byref(out)) == _lib.SA_EINVAL and not out
        assert e.lib.sa_window_range(e._h, base, base, None, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
        assert e.lib.sa_window_range(e._h, base, base, key, 1, 0, None) == _lib.SA_EINVAL
        _check_ranges(e, c)


@pytest.mark.parametrize("devices,rccl", [([0, 0], False), ([0, 0, 0], False), ([0], True)])
def test_group_equals_the_oracle_and_one_engine(devices, rccl):
    c, windows = case("group"), reference("group")
    (base, batch), = c.steps
    (first, last), = c.ranges
    assert last - first + 1 == 5 and c.cfg.n_windows == 16
    want = merged(windows, range(first, last + 1), c.keys)
    cfg = c.cfg
    gcfg = dataclasses.replace(cfg, options=OPT_GROUP_RCCL if rccl else OPT_GROUP_COPY)
    with Group(devices, gcfg) as g, Engine(cfg) as e:
        assert g.size == len(devices) and g.uses_rccl == rccl
        for x in (g, e):
            x.window_advance(base)
            x.ingest(batch)
        rg = g.window_range(first, last, c.keys, registers=True, cells=True)
        assert_range_equal(rg, want, cfg, "group")
        re_ = e.window_range(first, last, c.keys, registers=True, cells=True)
        for f in ("hist", "distinct", "hll", "cms", "errors"):
            assert np.array_equal(getattr(rg, f), getattr(re_, f)), f
        plain = g.window_range(first, last, c.keys)
        assert plain.hll is None and plain.cms is None
        assert np.array_equal(plain.hist, want.hist) and np.array_equal(plain.errors, want.errors)
        _raises(_lib.SA_ERANGE, lambda: g.window_range(base, base + 16))
        # the windows one by one still read as the oracle's
        hll, cms = windows[first]
        sk = g.window_read(first)
        assert np.array_equal(sk.hll, hll) and np.array_equal(sk.cms, cms)
