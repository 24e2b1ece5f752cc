"""Sliding series over the window ring (sa_window_series) against the CPU
oracle: for every window t of first..last the histogram of the registers
max-merged over t - width + 1 .. t, the point queries on those windows'
summed cells and the sum of their count-min row 0 -- bit-exact in hist, errors
and error_spans, and distinct is hll_estimate_hist of the histogram row
(tests/series_util.py builds the cases, the plans and the references;
tests/test_window_series_host.py proves the inputs can catch a wrong end of a
span, a missing ring mask, a swapped row and a wrong block seam).

  * every row of RING_ROWS (every ingest path and fold variant): the whole
    ring at width 1, width W, and width 2 where W >= 4;
  * moved:ring_512 (W = 4, wrapped): every valid (first, last, width);
  * moved:ring_1024_noerr (W = 32): widths 1, 2, 3, 5, 8, 16, 31, 32 over the
    largest span, width 5 also with 4, 5 and 6 outputs;
  * long (W = 256, 12 register columns a slot): widths 1, 7, 64, 100, 128, 129,
    255, 256, and the widths either side of the kernel's LDS-stash bound,
    32 | 33: up to width 32 a block's suffix maxima (width x 1 KiB for a tile
    of 64 columns) fit the 32 KiB stash and a window is read twice; from 33
    the block goes through the stash in chunks of 16 windows and is read
    three times.  That fallback keeps 64-column tiles up to width 256;
  * wide512 (W = 512, 40 columns a slot): widths 256 | 257 -- the tile goes
    from 64 columns to 32, two tiles a slot, the second of 8 columns -- and
    512;
  * hll_p 4 and 18: widths 1 and 2;
  * 0, 1 and 10,000 keys;
  * rows equal to window_range of the same engine;
  * idempotence, ordering behind an unsynchronised device ingest, and the
    reads that follow;
  * the error returns;
  * config C5 end to end: one series call flags exactly the injected windows.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
import series_util
from geometry_util import RING_ROWS, assert_geometry, check_against_oracle, key_pool
from ring_util import DeviceFeed
from series_util import PLANS, assert_series_equal, case, expected, reference
from spanagg import Config, Engine, SpanAggError, _lib
from spanagg.sketch import anomalous, heavy_hitters
from spanagg.synth import generate_c5

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


def _check_plan(e, c, plan):
    for first, last, width in plan:
        r = e.window_series(first, last, width, c.keys)
        assert_series_equal(r, expected(c.name, first, last, width), c.cfg, first, last, width, (first, last, width))
        assert np.array_equal(r.keys, c.keys)


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_whole_ring_on_every_path(row):
    e, c = _loaded(f"full:{row}")
    with e:
        W = c.cfg.n_windows
        assert sorted(w for _, _, w in PLANS[c.name]) == sorted({1, W} | ({2} if W >= 4 else set()))
        _check_plan(e, c, PLANS[c.name])


def test_every_series_of_a_moved_ring_of_four():
    e, c = _loaded("moved:ring_512")
    with e:
        assert len(PLANS[c.name]) == 20
        _check_plan(e, c, PLANS[c.name])
        first, last, width = c.base + 1, c.base + 3, 2
        r = e.window_series(first, last, width, c.keys)
        cms = np.sum([reference(c.name)[w][1].astype(np.uint64) for w in (last - 1, last)], axis=0, dtype=np.uint64)
        assert r.top_errors(2, 10) == heavy_hitters(cms, c.keys, 10)


def test_widths_around_the_blocks_of_a_moved_ring_of_32():
    e, c = _loaded("moved:ring_1024_noerr")
    with e:
        _check_plan(e, c, PLANS[c.name])


def test_long_ring_widths_and_the_stash_bounds():
    e, c = _loaded("long")
    with e:
        _check_plan(e, c, PLANS[c.name])
        # equality with the existing call: 16 outputs of the width-7 series, seams included
        first, last, width = c.base + 6, c.base + 255, 7
        r = e.window_series(first, last, width, c.keys)
        n_out = last - first + 1
        outs = sorted({0, 6, 7, 8, 13, 14, 15, n_out - 2, n_out - 1} | set(range(20, n_out - 2, 35)))[:16]
        assert len(outs) == 16
        for o in outs:
            t = first + o
            one = e.window_range(t - 6, t, c.keys)
            assert np.array_equal(r.hist[o], one.hist), t
            assert np.array_equal(r.errors[o], one.errors), t
            assert np.array_equal(r.distinct[o], one.distinct), t


def test_widths_past_256_take_narrower_tiles():
    e, c = _loaded("wide512")
    with e:
        _check_plan(e, c, PLANS[c.name])


@pytest.mark.parametrize("name", list(series_util.range_util.EXTREMES))
def test_extremes_of_hll_p(name):
    e, c = _loaded(name)
    with e:
        _check_plan(e, c, PLANS[name])


def test_key_counts():
    e, c = _loaded("moved:ring_512")
    with e:
        first, last, width = c.base + 1, c.base + 3, 2
        want = expected(c.name, first, last, width)
        none = e.window_series(first, last, width)
        assert none.errors.shape == (3, 0) and none.keys.shape == (0,) and none.top_errors(0) == []
        assert np.array_equal(none.hist, want.hist) and np.array_equal(none.error_spans, want.error_spans)
        one = e.window_series(first, last, width, c.keys[:1])
        assert np.array_equal(one.errors, want.errors[:, :1]) and want.errors[:, 0].all()
        rng = np.random.default_rng(10_000)
        many = np.concatenate([key_pool(RING_ROWS["ring_512"]["n_keys"]), np.zeros(1, np.uint64),
                               rng.integers(0, 2**64, 10_000, dtype=np.uint64)])[:10_000]
        r = e.window_series(first, last, width, many)
        ref = series_util.series(reference(c.name), first, last, width, many)
        assert r.errors.shape == (3, 10_000) and np.array_equal(r.errors, ref.errors)
        assert np.array_equal(r.hist, want.hist)


def test_idempotent_and_ordered_behind_a_device_ingest():
    c = case("full:ring_512")
    (base, batch), = c.steps
    first, last, width = base + 1, base + 3, 2
    want = expected(c.name, first, last, width)
    with Engine(c.cfg) as e:
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_series"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_series(first, last, width, c.keys)
        assert_series_equal(r, want, c.cfg, first, last, width, "behind the ingest")
        again = e.window_series(first, last, width, c.keys)
        for f in ("hist", "distinct", "error_spans", "errors"):
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
        _raises(_lib.SA_ERANGE, lambda: e.window_series(base + 1, base, 1))
        _raises(_lib.SA_ERANGE, lambda: e.window_series(base, base, 0))
        _raises(_lib.SA_ERANGE, lambda: e.window_series(base + W - 1, base + W - 1, W + 1))
        _raises(_lib.SA_ERANGE, lambda: e.window_series(base, base + 1, 2))  # first - width + 1 below the base
        _raises(_lib.SA_ERANGE, lambda: e.window_series(base, base + W, 1))
        out = C.POINTER(_lib.sa_series_result)()
        key = (C.c_uint64 * 1)(5)
        call = e.lib.sa_window_series
        assert call(e._h, 1, 1, 3, None, 0, 0, C.byref(out)) == _lib.SA_ERANGE and not out  # first + 1 < width
        assert call(e._h, base, base, 1, None, 0, 1, C.byref(out)) == _lib.SA_EINVAL and not out
        assert call(e._h, base, base, 1, None, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
        assert call(e._h, base, base, 1, key, 1, 0, None) == _lib.SA_EINVAL
        _check_plan(e, c, PLANS[c.name])


def test_c5_detection_from_one_series_call():
    c5 = generate_c5(300_000)
    S = c5.base.n_services
    o = pyoracle.Oracle(n_services=S)
    o.ingest(c5.base.batch)
    windows = {w: o.window(w) for w in o.window_ids()}
    first, n = c5.first_window, c5.n_windows
    assert n == 60 and sorted(windows) == list(range(first, first + n))
    ekeys = np.array([int(c5.base.key_hashes[i]) for i, (svc, _, _, st) in enumerate(c5.base.key_strings)
                      if st == 2 and svc == "payment"], dtype=np.uint64)
    with Engine(Config(n_windows=64, key_capacity=1000, n_services=S)) as e:
        e.window_advance(first)
        e.ingest(c5.base.batch)
        r = e.window_series(first, first + 59, 1, ekeys)
        lo, hi = c5.error_windows
        assert anomalous(r.errors.sum(axis=1), factor=5.0) == list(range(lo, hi + 1))
        blo, bhi = c5.burst_windows
        assert anomalous(r.distinct[:, c5.burst_service], factor=2.0, min_base=10.0) == list(range(blo, bhi + 1))
        for i in range(n):
            assert int(r.error_spans[i]) == int(windows[first + i][1].astype(np.uint64).sum(axis=1)[0]), i
        assert_series_equal(r, series_util.series(windows, first, first + 59, 1, ekeys), e.config, first, first + 59, 1,
                            "c5 width 1")
        six = e.window_series(first + 5, first + 59, 6, ekeys)
        assert_series_equal(six, series_util.series(windows, first + 5, first + 59, 6, ekeys), e.config, first + 5,
                            first + 59, 6, "c5 width 6")
        t = first + 17
        m = series_util.range_util.merged(windows, range(t - 5, t + 1), ekeys)
        assert np.array_equal(six.hist[12], m.hist) and np.array_equal(six.errors[12], m.errors)
