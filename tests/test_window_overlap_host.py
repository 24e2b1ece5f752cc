"""sa_window_overlap on the CPU: what the workloads of tests/overlap_util.py
can catch, shown on the oracle alone, and the library surface that needs no
GPU.  tests/test_gpu_window_overlap.py runs the same cases through the kernels.

  * pair rows are telling: a graded pair's row differs from both services'
    own histograms, and different pairs have different rows -- a wrong pair
    index and a missing maximum would both show;
  * order matters: pairing inside each window -- no window's pair row is the
    merged arrays', and the per-window shared estimates added up are not the
    merged arrays' -- for most pairs;
  * range ends matter: a range short of its last window changes rows;
  * the planted identical pair and the empty service;
  * against the true set sizes, computed from the trace ids: for every pair
    |shared - truth| <= 3 x 1.04 / sqrt(2^p) x (|A| + |B| + |A u B|), the sum of
    the three estimates' standard errors, each at three sigma;
  * the symbols, the null-handle returns and the constants.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import overlap_util as ou
import spanagg
from overlap_util import PLANT, case, expected, pair_index, reference, truth
from spanagg import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _full(name):
    c = case(name)
    (first, last), = c.ranges if name != "moved" else [c.ranges[c.cfg.n_windows - 1]]
    wins = range(first, last + 1)
    return c, reference(name), wins, list(range(c.cfg.n_services))


def _graded(S):
    """Pairs of the rest close enough to share runs."""
    return [(i, j) for i in range(PLANT.REST, S) for j in range(i + 1, min(S, i + 8))]


def test_pair_rows_are_telling():
    c, windows, wins, svcs = _full("p8x64")
    want = expected(windows, wins, svcs, c.cfg.hll_p)
    n = len(svcs)
    graded = _graded(n)
    assert len(graded) > 300
    for i, j in graded:
        row = want.pair_hist[pair_index(i, j, n)]
        assert not np.array_equal(row, want.hist[i]) and not np.array_equal(row, want.hist[j]), (i, j)
        assert j > i + 1 or want.shared[i, j] > 0.3 * want.distinct[i]  # neighbours share most of their traces
    # every pair outside the planted repeats (the empty service's pair rows are the other's own
    # histogram, the second of the identical two repeats the first) has a row of its own
    skip = {PLANT.EMPTY, PLANT.SAME[1]}
    rows = [want.pair_hist[pair_index(i, j, n)].tobytes() for i in range(n) for j in range(i + 1, n)
            if i not in skip and j not in skip]
    assert len(rows) == 62 * 61 // 2 == len(set(rows))


def test_order_matters():
    """Merge, then pair.  Pairing inside a window misses the traces that meet
    the two services in different windows."""
    c, windows, wins, svcs = _full("p8x64")
    p, n = c.cfg.hll_p, len(svcs)
    want = expected(windows, wins, svcs, p)
    per_window = [expected(windows, [w], svcs, p) for w in wins]
    graded = _graded(n)
    other_rows = other_sums = 0
    for i, j in graded:
        k = pair_index(i, j, n)
        other_rows += all(not np.array_equal(w.pair_hist[k], want.pair_hist[k]) for w in per_window)
        other_sums += sum(w.shared[i, j] for w in per_window) != want.shared[i, j]
    assert other_rows > 0.9 * len(graded) and other_sums > 0.9 * len(graded), (other_rows, other_sums, len(graded))
    # and the planted shared traces do cross windows: inside single windows the identical two are not identical
    a, b = PLANT.SAME
    assert any(not np.array_equal(windows[w][0][a], windows[w][0][b]) for w in wins)


def test_range_ends_matter():
    c = case("moved")
    windows, p = reference("moved"), c.cfg.hll_p
    svcs, W = list(range(c.cfg.n_services)), c.cfg.n_windows
    full = expected(windows, range(c.base, c.base + W), svcs, p)
    for wins in (range(c.base, c.base + W - 1), range(c.base + 1, c.base + W)):
        short = expected(windows, wins, svcs, p)
        changed = (short.pair_hist != full.pair_hist).any(axis=1)
        live = [pair_index(i, j, len(svcs)) for i in range(1, len(svcs)) for j in range(i + 1, len(svcs))]
        assert changed[live].all(), wins
    # the windows the advance retired are gone: the ring's first windows hold the second batch alone
    assert len(c.ranges) == W * (W + 1) // 2


@pytest.mark.parametrize("name", ["p8x64", "p14x200"])
def test_planted_cases(name):
    """(Not on the moved ring: the windows its advance retired took some of the
    planted traces' spans with them, one service's and not the other's.)"""
    c, windows, wins, svcs = _full(name)
    if name == "p14x200":
        svcs = list(range(8)) + [150]
    want = expected(windows, wins, svcs, c.cfg.hll_p)
    n = len(svcs)
    a, b = PLANT.SAME
    row = want.pair_hist[pair_index(a, b, n)]
    assert np.array_equal(row, want.hist[a]) and np.array_equal(row, want.hist[b])
    assert want.shared[a, b] == want.distinct[a] == want.distinct[b] > 0
    e = PLANT.EMPTY
    assert want.hist[e, 0] == 1 << c.cfg.hll_p and want.distinct[e] == 0.0
    for j in range(1, n):
        assert want.union[e, j] == want.distinct[j] and want.shared[e, j] == 0.0, j
    # the subset: the union is the superset's own sketch
    assert np.array_equal(want.pair_hist[pair_index(PLANT.SUB, PLANT.SUP, n)], want.hist[PLANT.SUP])
    # ((d_sub + d_sup) - d_sup: d_sub up to the sum's rounding)
    assert abs(want.shared[PLANT.SUB, PLANT.SUP] - want.distinct[PLANT.SUB]) <= 1e-12 * want.distinct[PLANT.SUP]
    assert want.distinct[PLANT.SUB] < want.distinct[PLANT.SUP]


@pytest.mark.parametrize("name,svcs", [("p4", None), ("p18", None), ("p8x64", None), ("moved", None),
                                       ("p14x200", ou.SEL5), ("p14x200", ou.SEL9)])
def test_against_the_true_set_sizes(name, svcs):
    c, windows, wins, every = _full(name)
    svcs = list(svcs or every)
    p = c.cfg.hll_p
    want = expected(windows, wins, svcs, p)
    sets = truth(c, wins[0], wins[-1])
    se = 1.04 / np.sqrt(2.0 ** p)
    worst = 0.0
    for i in range(len(svcs)):
        A = sets[svcs[i]]
        for j in range(i + 1, len(svcs)):
            B = sets[svcs[j]]
            both = len(A & B)
            bound = 3 * se * (len(A) + len(B) + (len(A) + len(B) - both))
            err = abs(want.shared[i, j] - both)
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (name, svcs[i], svcs[j], want.shared[i, j], both, bound)
    print(f"{name}: worst |shared - truth| / bound = {worst:.3f}")
    if name == "p18":  # half the traces on both services, and a narrow counter would wrap
        assert abs(len(sets[0] & sets[1]) / len(sets[0] | sets[1]) - 0.5) < 0.01
        assert want.pair_hist.max() > 65535 and want.hist.max() > 65535


def test_library_surface():
    lib = spanagg.load()
    header = open(os.path.join(ROOT, "include", "spanagg.h")).read()
    for sym in ("sa_window_overlap", "sa_group_window_overlap", "sa_overlap_result_free"):
        assert hasattr(lib, sym) and re.search(r"\b%s\(" % sym, header), sym
    out = C.POINTER(_lib.sa_overlap_result)()
    ids = (C.c_uint32 * 2)(0, 1)
    assert lib.sa_window_overlap(None, 0, 0, ids, 2, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    assert lib.sa_group_window_overlap(None, 0, 0, ids, 2, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    lib.sa_overlap_result_free(None)
    m = re.search(r"#define SA_OVERLAP_MAX_SERVICES (\d+)u", header)
    assert int(m.group(1)) == _lib.SA_OVERLAP_MAX_SERVICES == _lib.OVERLAP_MAX_SERVICES == spanagg.OVERLAP_MAX_SERVICES == 64
    assert C.sizeof(_lib.sa_overlap_result) == 16 + 4 * 4 + 6 * C.sizeof(C.c_void_p)
    assert {"OverlapResult", "OVERLAP_MAX_SERVICES"} <= set(spanagg.__all__)
