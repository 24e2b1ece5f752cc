"""Movers without a GPU: on the oracle alone, that the inputs of
tests/test_gpu_window_movers.py (movers_util) can catch the mistakes the
kernels can make, that movers_util.movers() -- the vectorised reference -- is
sketch.movers, and that the library exports the call.

  * ring_binned's halves: tens of thousands of rises and of falls, the cuts at
    k = 10 and k = SA_TOP_MAX_K both inside a tie class, so the device has to
    select and the tie-break decides; reversing it changes the answer;
  * ties_binned's halves: a handful of distinct scores over thousands of keys;
  * ring_512's halves: fewer matches than SA_TOP_MAX_K, everything is returned;
  * swapping the ranges is the fall, with baseline and current exchanged;
  * ranges of unequal length: ranking by current - baseline (no normalisation)
    and by current alone (sa_window_top of the current range) give other lists;
  * a planted incident comes out on top, by a wide margin.
"""
import ctypes as C

import numpy as np
import pytest

import movers_util as mu
import top_util
from spanagg import SA_MOVERS_FALL, TOP_MAX_K, _lib
from spanagg import sketch
from movers_util import candidates, case, cells, movers, ranked, reference, scores, split
from top_util import tie_class


def _whole(name):
    c = case(name)
    return c, reference(name), candidates([b for _, b in c.steps])


def test_symbols_and_null_engine():
    lib = _lib.load()
    for name in ("sa_window_movers", "sa_group_window_movers", "sa_movers_result_free"):
        assert hasattr(lib, name), name
    out = C.POINTER(_lib.sa_movers_result)()
    assert lib.sa_window_movers(None, 0, 0, 0, 0, 10, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    assert lib.sa_group_window_movers(None, 0, 0, 0, 0, 10, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    lib.sa_movers_result_free(None)
    assert _lib.SA_MOVERS_FALL == SA_MOVERS_FALL == 1


@pytest.mark.parametrize("name", ["full:ring_512", "ties_binned", "group"])
@pytest.mark.parametrize("fall", [False, True])
def test_the_reference_is_sketch_movers(name, fall):
    c, windows, cand = _whole(name)
    base, cur = ((c.base + 1, c.base + 3), (c.base + 4, c.base + 5)) if name == "group" else split(c)
    nb, nc = base[1] - base[0] + 1, cur[1] - cur[0] + 1
    cb, cc = cells(windows, *base), cells(windows, *cur)
    everything = sketch.movers(cb, cc, nb, nc, cand, len(cand), fall=fall)
    assert len(everything) > 10
    for k in (1, 10, TOP_MAX_K):
        want = movers(windows, base, cur, cand, k, fall=fall)
        assert mu.items(want) == everything[:k], k
        assert (want.n_resident, want.n_matched) == (len(cand), len(everything))
        assert (want.error_spans_base, want.error_spans_cur) == (int(cb[0].sum()), int(cc[0].sum()))
    floor = everything[len(everything) // 2][1]
    some = sketch.movers(cb, cc, nb, nc, cand, len(cand), min_score=floor, fall=fall)
    assert some == [r for r in everything if r[1] >= floor]
    assert mu.items(movers(windows, base, cur, cand, len(cand), min_score=floor, fall=fall)) == some
    assert sketch.movers(cb, cc, nb, nc, cand, 10, min_score=0, fall=fall) == everything[:10]


def _halves(name, fall):
    c, windows, cand = _whole(name)
    base, cur = split(c)
    W = c.cfg.n_windows
    assert base[1] - base[0] + 1 == cur[1] - cur[0] + 1 == W // 2 and base[1] < cur[0]
    _, _, s = scores(cells(windows, *base), cells(windows, *cur), W // 2, W // 2, cand, fall)
    order = ranked(s, cand)
    return cand, s, order, ranked(s, cand, reverse_ties=True)


@pytest.mark.parametrize("fall,matched", [(False, 26_057), (True, 25_064)])
def test_binned_halves_select_and_cut_inside_tie_classes(fall, matched):
    cand, s, order, other = _halves("full:ring_binned", fall)
    assert len(cand) == 57_646 and len(order) == matched > 4 * TOP_MAX_K  # the select has work
    for k in (10, TOP_MAX_K):
        start, size = tie_class(s[order], k)
        assert s[order][k - 1] == s[order][k] and start < k < start + size, (k, start, size)
        assert not np.array_equal(cand[order[:k]], cand[other[:k]]), k  # the tie-break decides


def test_tie_case_halves_have_few_distinct_scores():
    cand, s, order, other = _halves("ties_binned", False)
    assert len(order) == 18_958 and len(np.unique(s[order])) == 8
    for k in (10, top_util.TIES_BINNED_K, TOP_MAX_K):
        start, size = tie_class(s[order], k)
        assert s[order][k - 1] == s[order][k] and start < k < start + size, (k, start, size)
        assert not np.array_equal(cand[order[:k]], cand[other[:k]]), k


def test_small_ring_halves_return_everything():
    rises, falls = _halves("full:ring_512", False), _halves("full:ring_512", True)
    assert (len(rises[2]), len(falls[2])) == (265, 273) and max(265, 273) < TOP_MAX_K
    assert not set(rises[0][rises[2]]) & set(falls[0][falls[2]])  # a series rises or falls, never both
    assert len(rises[2]) + len(falls[2]) + int((rises[1] == 0).sum()) == len(rises[0])


@pytest.mark.parametrize("name", ["full:ring_512", "planted", "moved:ring_512"])
def test_swapped_ranges_are_the_fall(name):
    c, windows, cand = _whole(name)
    base, cur = ((c.base, c.base + 2), (c.base + 3, c.base + 3)) if name.startswith("moved") else split(c)
    for k in (10, TOP_MAX_K):
        a, b = movers(windows, base, cur, cand, k, fall=True), movers(windows, cur, base, cand, k)
        assert len(a.keys) > 3 and np.array_equal(a.keys, b.keys) and np.array_equal(a.score, b.score)
        assert np.array_equal(a.baseline, b.current) and np.array_equal(a.current, b.baseline)
        assert (a.n_matched, a.error_spans_base, a.error_spans_cur) == (b.n_matched, b.error_spans_cur, b.error_spans_base)
        rise = movers(windows, base, cur, cand, k)
        assert not set(rise.keys) & set(a.keys)


def test_wrong_normalisation_and_a_missing_baseline_show():
    """moved:ring_512, a 3-window baseline against a 1-window current range."""
    c, windows, cand = _whole("moved:ring_512")
    base, cur = (c.base, c.base + 2), (c.base + 3, c.base + 3)
    cb, cc = cells(windows, *base), cells(windows, *cur)
    b, cu, s = scores(cb, cc, 3, 1, cand)
    want = movers(windows, base, cur, cand, 10)
    assert np.array_equal(want.score, 3 * want.current.astype(np.int64) - want.baseline.astype(np.int64))
    assert len(want.keys) == 10 < want.n_matched
    # current - baseline: the longer baseline outweighs every rise
    plain = cu.astype(np.int64) - b.astype(np.int64)
    assert not np.array_equal(cand[ranked(plain, cand)[:10]], want.keys)
    assert len(ranked(plain, cand)) < want.n_matched
    # the length of the wrong range: other scores, another list
    _, _, swapped = scores(cb, cc, 1, 3, cand)
    assert not np.array_equal(cand[ranked(swapped, cand)[:10]], want.keys)
    # current alone -- sa_window_top of the current range -- is led by the series that always fail most
    assert not np.array_equal(top_util.top(cc, cand, 10).keys, want.keys)
    c5, w5, cand5 = _whole("full:ring_512")
    b5, c5r = split(c5)
    assert not np.array_equal(top_util.top(cells(w5, *c5r), cand5, 10).keys, movers(w5, b5, c5r, cand5, 10).keys)


def test_planted_incident_leads_by_a_wide_margin():
    c, windows, cand = _whole("planted")
    base, cur = split(c)
    W = c.cfg.n_windows
    assert (base, cur) == ((c.base, c.base + W - 2), (c.base + W - 1, c.base + W - 1)) and W == 4
    planted = mu.planted_keys()
    assert len(planted) == 3 and np.isin(planted, cand).all()
    want = movers(windows, base, cur, cand, 10)
    assert set(want.keys[:3]) == set(planted) and want.n_matched > 10
    # about 940 spans of each in the last window, all ERROR, against 1 in 20 before
    assert int(want.score[2]) > 2000 > 20 * int(want.score[3]) > 0, want.score[:4]
    # with this seed two of the three tie: the key order decides between them
    assert [int(s) for s in want.score[:4]] == [2755, 2755, 2595, 31] and want.keys[0] < want.keys[1]
    assert (want.current[:3] > 800).all() and (want.baseline[:3] < 250).all()
    assert np.array_equal(want.score[:3], 3 * want.current[:3].astype(np.int64) - want.baseline[:3].astype(np.int64))
    # the fall does not show them
    assert not np.isin(planted, movers(windows, base, cur, cand, TOP_MAX_K, fall=True).keys).any()
