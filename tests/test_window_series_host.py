"""Sliding series without a GPU: on the oracle alone, that the inputs of every
series tests/test_gpu_window_series.py asks for (series_util.PLANS) can catch
the mistakes the kernels can make, and that series_util.series() -- the
vectorised reference the GPU test compares against -- is range_util.merged()
output by output.

For every case and every (first, last, width) of its plan, at the checked
outputs (series_util.checked: first, last, the block seams j * width - 1,
j * width, j * width + 1, the spans that pass the slot wrap):

  * series() equals merged() there in histogram and errors;
  * the reference at width w differs in some histogram from the references at
    w - 1 and w + 1 for the same output: both ends of the span show;
  * where the span passes the slot wrap, the walk without the ring mask
    (range_util.unmasked) gives another histogram and other errors;
  * over the whole series some key's errors differ between every two
    consecutive outputs, so a swapped row shows.
"""
import numpy as np
import pytest

import range_util
import series_util
from series_util import PLANS, case, checked, expected, hist_of, reference


def test_the_plans_cover_what_the_issue_lists():
    assert set(PLANS) == {f"full:{r}" for r in range_util.RING_ROWS} | {"moved:ring_512", "moved:ring_1024_noerr",
                                                                        "long", "wide512", "p4", "p18"}
    assert len(PLANS["moved:ring_512"]) == 20  # every valid (first, last, width) of four windows
    assert [w for _, _, w in PLANS["full:ring1"]] == [1]
    assert sorted(w for _, _, w in PLANS["full:ring_512"]) == [1, 2, 4]
    noerr = PLANS["moved:ring_1024_noerr"]
    assert sorted({w for _, _, w in noerr}) == list(series_util.NOERR_WIDTHS)
    assert sorted(l - f + 1 for f, l, w in noerr if w == 5)[:3] == [4, 5, 6]  # below, at and above one block
    assert {1, 7, 64, 100, 255, 256, 32, 33} <= {w for _, _, w in PLANS["long"]}


def test_columns_are_the_point_querys():
    from spanagg.sketch import cms_query
    keys = case("p4").keys
    cols = series_util.columns(keys, 4, 2048)
    cms = np.arange(4 * 2048, dtype=np.uint64).reshape(4, 2048)
    for i, k in enumerate(keys):
        assert cms_query(cms, int(k)) == int(min(cms[r, cols[r, i]] for r in range(4)))


def test_long_markers_raise_the_registers_they_are_built_for():
    import struct

    import pyoracle
    cfg, base = series_util.LONG_CFG, case("long").base
    mk, windows = series_util.long_markers(cfg, base), reference("long")
    assert len(mk) == 256
    for k in (0, 63, 64, 191, 192, 255):
        x = pyoracle.xxh64(struct.pack("<QQ", int(mk.trace_w0[k]), int(mk.trace_w1[k])))
        assert x >> 58 == k % 64 and int(mk.meta[k]) & 0xFFFF == (k % 192) // 64
        want = 41 if k < 192 else 40
        hll = windows[base + k][0]
        assert int(hll[(k % 192) // 64, k % 64]) == want and int(hll.max()) == want and (hll == want).sum() == 1
    assert max(int(windows[w][0].max()) for w in windows) == 41


def test_seams_are_among_the_checked_outputs():
    got = set(checked(100, 130, 5, 32))  # 31 outputs: blocks start at outputs 5, 10 .. 30
    for j in range(1, 7):
        assert {100 + j * 5 + k for k in (-1, 0, 1) if j * 5 + k <= 30} <= got, j
    assert {100, 130} <= got
    for first, last, width in PLANS["long"]:
        ts = set(checked(first, last, width, 256))
        if last - first + 1 > width + 1:
            assert {first + width - 1, first + width, first + width + 1} <= ts, width


@pytest.mark.parametrize("name", list(PLANS))
def test_case_inputs_can_catch_a_wrong_series(name):
    c, windows = case(name), reference(name)
    W, base = c.cfg.n_windows, c.base
    wrapped = 0
    for first, last, width in PLANS[name]:
        a = first - width + 1
        assert base <= a and first <= last < base + W and 1 <= width <= W, (first, last, width)
        want = expected(name, first, last, width)
        assert want.hist[:, :, 1:].any() and want.errors.any() and want.error_spans.any()
        for t in checked(first, last, width, W):
            i, wins = t - first, list(range(t - width + 1, t + 1))
            m = range_util.merged(windows, wins, c.keys)
            assert np.array_equal(want.hist[i], m.hist), (first, last, width, t)
            assert np.array_equal(want.errors[i], m.errors), (first, last, width, t)
            assert int(want.error_spans[i]) == int(m.cms[0].sum()), (first, last, width, t)
            if width > 1:  # the span without its first window
                assert not np.array_equal(m.hist, hist_of(windows, wins[1:])), (first, last, width, t, "w - 1")
            if width < W and t - width >= base:  # the span with the window before it
                assert not np.array_equal(m.hist, hist_of(windows, [t - width] + wins)), (first, last, width, t, "w + 1")
            cut = range_util.unmasked(wins[0], t, W)
            if cut is not None:
                wrapped += 1
                other = range_util.merged(windows, cut, c.keys)
                assert not np.array_equal(m.hist, other.hist) and not np.array_equal(m.errors, other.errors), \
                    (first, last, width, t, "no mask")
        # consecutive rows differ in some key
        assert (want.errors[1:] != want.errors[:-1]).any(axis=1).all(), (first, last, width)
        assert (want.hist[1:] != want.hist[:-1]).any(axis=(1, 2)).all(), (first, last, width)
    if name.startswith("moved:") or name in series_util.OWN:
        assert wrapped >= 3, "the series must pass the slot wrap"
