"""Heavy hitters without a GPU: on the oracle alone, that the inputs of
tests/test_gpu_window_top.py (top_util) can catch the mistakes the kernels can
make, that top_util.top() -- the vectorised reference -- is sketch.heavy_hitters
with cms_query, and that the library exports the call.

  * the tie cases cut inside a tie class: the k-th and (k + 1)-th estimates are
    equal and the class is larger than what remains of k, so the tie-break
    decides; reversing it changes the answer;
  * ties_binned's class has thousands of keys and the matches pass the 4,096
    pairs one workgroup sorts, so the device has to select;
  * the ring rows with 60,000 keys (ring_binned and ring_dense among them)
    have more matches than SA_TOP_MAX_K, the small rows fewer;
  * a table of 4,096 slots holds fewer matches than SA_TOP_MAX_K, one of 8,192
    more, with a tie at the cut;
  * every two sub-ranges of the moved ring give different lists;
  * a key that is queried but was never ingested would appear: without the
    candidate filter the answer changes.
"""
import ctypes as C

import numpy as np
import pytest

import top_util
from geometry_util import RING_ROWS
from range_util import query_keys
from spanagg import TOP_MAX_K, _lib
from spanagg.sketch import heavy_hitters
from top_util import TIES_BINNED_K, TIES_SMALL_KS, candidates, case, cells, ranked, reference, tie_class, top


def _whole(name):
    c = case(name)
    (first, last), = c.ranges
    return c, cells(reference(name), first, last), candidates([b for _, b in c.steps])


def test_symbols_and_null_engine():
    lib = _lib.load()
    for name in ("sa_window_top", "sa_group_window_top", "sa_top_result_free"):
        assert hasattr(lib, name), name
    out = C.POINTER(_lib.sa_top_result)()
    assert lib.sa_window_top(None, 0, 0, 10, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    assert lib.sa_group_window_top(None, 0, 0, 10, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    lib.sa_top_result_free(None)
    assert TOP_MAX_K == top_util.TOP_MAX_K == _lib.SA_TOP_MAX_K == 4096


@pytest.mark.parametrize("name", ["ties_small", "ties_binned", "full:ring_512", "cells1m", "group"])
def test_the_reference_is_heavy_hitters(name):
    c, cms, cand = _whole(name)
    hh = heavy_hitters(cms, cand, TOP_MAX_K)
    for k in (1, 10, TOP_MAX_K):
        want = top(cms, cand, k)
        assert top_util.items(want) == hh[:k], k
        assert want.n_resident == len(cand) and want.n_matched == sum(1 for _ in heavy_hitters(cms, cand, len(cand)))
        assert want.error_spans == int(cms[0].sum())


def test_small_ties_cut_inside_a_class():
    c, cms, cand = _whole("ties_small")
    assert (c.cfg.cms_d, c.cfg.cms_w) == (1, 2) and len(cand) == 1050
    keys, est = ranked(cms, cand)
    assert len(np.unique(est)) == 2 and len(keys) == len(cand)  # two tie classes of the whole table
    other, _ = ranked(cms, cand, reverse_ties=True)
    for k in TIES_SMALL_KS[:-1]:
        start, size = tie_class(est, k)
        assert est[k - 1] == est[k] and size > k - start, k
        assert not np.array_equal(keys[:k], other[:k]), k
    assert TIES_SMALL_KS[-1] == TOP_MAX_K > len(keys)  # everything is returned, sorted


def test_binned_ties_cut_inside_a_class_of_thousands():
    c, cms, cand = _whole("ties_binned")
    assert (c.cfg.cms_d, c.cfg.cms_w) == (2, 64) and len(cand) > 50_000
    keys, est = ranked(cms, cand)
    assert len(keys) > 10 * TOP_MAX_K
    other, _ = ranked(cms, cand, reverse_ties=True)
    for k in (TIES_BINNED_K, TOP_MAX_K):
        start, size = tie_class(est, k)
        assert est[k - 1] == est[k] and size >= 4000 and start < k < start + size, (k, start, size)
        assert not np.array_equal(keys[:k], other[:k]), k
    assert est[9] == est[10]  # k = 10 cuts a class too


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_ring_rows_on_both_sides_of_the_largest_k(row):
    c, cms, cand = _whole(f"full:{row}")
    want = top(cms, cand, TOP_MAX_K)
    assert want.n_matched > 10 and want.error_spans > 0
    assert (RING_ROWS[row]["n_keys"] == 60_000) == (row in ("ring_part", "ring_atomic", "ring_binned", "ring_dense"))
    if RING_ROWS[row]["n_keys"] == 60_000:  # the HBM tables
        assert want.n_matched > TOP_MAX_K == len(want.keys)  # the cut is inside the list
    else:
        assert want.n_matched < TOP_MAX_K and len(want.keys) == want.n_matched


def test_table_sizes_on_both_sides_of_the_select():
    c, cms, cand = _whole("slots4096")
    assert 2048 < len(cand) < 1.25 * c.cfg.key_capacity <= 4096 == TOP_MAX_K  # a table of 4,096 slots
    c, cms, cand = _whole("slots8192")
    assert 4096 < 1.25 * c.cfg.key_capacity <= 8192
    want = top(cms, cand, TOP_MAX_K)
    assert TOP_MAX_K < want.n_matched < len(cand) and want.errors[-1] == want.errors[-2]


def test_sub_ranges_of_the_moved_ring_differ():
    c, windows = case("moved:ring_512"), reference("moved:ring_512")
    cand = candidates([b for _, b in c.steps])
    assert len(c.ranges) == 10
    lists = {(first, last): top_util.items(top(cells(windows, first, last), cand, 10)) for first, last in c.ranges}
    assert all(len(v) == 10 for v in lists.values())
    assert len({tuple(v) for v in lists.values()}) == len(lists)
    # the keys of both batches are candidates, the retired windows' errors are gone
    assert len(cand) == len(candidates([c.steps[0][1]])) == len(candidates([c.steps[1][1]]))


def test_the_candidate_filter_shows():
    c, cms, cand = _whole("ties_small")
    fresh = query_keys(cand, 5)[200:299]
    assert len(fresh) == 99 and not np.isin(fresh, cand).any()
    for k in (64, 500, TOP_MAX_K):
        with_fresh = heavy_hitters(cms, np.concatenate([cand, fresh]), k)
        assert with_fresh != top_util.items(top(cms, cand, k)), k
    # on the default sketch a series never ingested mostly reads 0: the reclaim
    # test queries keys that were ingested, and are no longer resident
    _, cms4, cand4 = _whole("full:ring_512")
    assert top(cms4, cand4[:50], TOP_MAX_K).n_matched == 50 < top(cms4, cand4, TOP_MAX_K).n_matched
