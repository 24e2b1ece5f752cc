"""Window-range queries without a GPU: the histogram estimator
(sa_hll_estimate_hist), and -- on the oracle alone -- that the inputs of every
case of tests/test_gpu_window_range.py (tests/range_util.py) can catch an
off-by-one at either end of the range, a missing merge and a missing wrap."""
import math

import numpy as np
import pytest

import range_util
from spanagg import hll_estimate, hll_estimate_hist


def _alpha(m):
    return {16: 0.673, 32: 0.697, 64: 0.709}.get(m, 0.7213 / (1.0 + 1.079 / m))


def _restated(hist, p):
    """(estimate, raw estimate): sum hist[v] * 2^-v as one exact integer,
    rounded to a double once; then sa_hll_estimate's alpha and branch."""
    m = 1 << p
    s = float(sum(int(hist[v]) << (63 - v) for v in range(64))) / 2 ** 63
    raw = _alpha(m) * m * m / s
    zeros = int(hist[0])
    return (m * math.log(m / zeros) if raw <= 2.5 * m and zeros else raw), raw


def _register_arrays(p):
    """Drawn arrays from nearly empty (the linear-counting branch) to full,
    then all zero and all 61."""
    m = 1 << p
    rng = np.random.default_rng([p, 0x5EED])
    for fill in (0.02, 0.5, 1.0):
        rho = np.minimum(rng.geometric(0.5, m), 65 - p)
        yield np.where(rng.random(m) < fill, rho, 0).astype(np.uint8)
    for load in (3, 40):  # registers after load * m distinct values: each the largest of `load` draws
        yield np.minimum(rng.geometric(0.5, (load, m)).max(axis=0), 65 - p).astype(np.uint8)
    yield np.zeros(m, np.uint8)
    yield np.full(m, 61, np.uint8)


@pytest.mark.parametrize("p", [4, 11, 14, 18])
def test_estimate_hist_is_the_exact_sum_and_agrees_with_the_register_estimate(p):
    m = 1 << p
    for i, regs in enumerate(_register_arrays(p)):
        hist = np.bincount(regs, minlength=64).astype(np.uint32)
        want, raw = _restated(hist, p)
        # the branch cannot flip between the two summations
        assert abs(raw / (2.5 * m) - 1.0) > 1e-6, (p, i)
        assert hll_estimate_hist(hist, p) == want, (p, i)
        # sa_hll_estimate sums at most 2^18 positive terms in sequence: off by
        # at most 2^18 * 2^-53 = 2.9e-11 relative
        assert hll_estimate_hist(hist, p) == pytest.approx(hll_estimate(regs, p), rel=1e-10, abs=0), (p, i)


def test_estimate_hist_rejects_a_bad_p():
    hist = np.zeros(64, np.uint32)
    hist[0] = 8
    assert hll_estimate_hist(hist, 3) == -1.0
    assert hll_estimate_hist(hist, 19) == -1.0


def _differs(a, b):
    return not np.array_equal(a.hist, b.hist) and not np.array_equal(a.errors, b.errors)


@pytest.mark.parametrize("name", range_util.CASES)
def test_case_inputs_can_catch_a_wrong_range(name):
    """For every range the GPU test asks for: the merged histogram and the
    errors vector both differ from those of the range without its first
    window, without its last, of the last window alone, and of the walk
    without the ring mask where the range wraps."""
    c, windows = range_util.case(name), range_util.reference(name)
    W = c.cfg.n_windows
    wrapped = 0
    for first, last in c.ranges:
        assert c.base <= first <= last < c.base + W
        wins = list(range(first, last + 1))
        want = range_util.merged(windows, wins, c.keys)
        assert (want.hist.sum(axis=1) == 1 << c.cfg.hll_p).all()
        assert want.hist[:, 1:].any() and want.errors.any(), (first, last)  # something to merge
        assert int(want.cms.max()) < 2 ** 32
        if len(wins) == 1:
            continue
        for what, other in (("no first", wins[1:]), ("no last", wins[:-1]), ("last alone", wins[-1:])):
            assert _differs(want, range_util.merged(windows, other, c.keys)), (first, last, what)
        cut = range_util.unmasked(first, last, W)
        if cut is not None:
            wrapped += 1
            assert 0 < len(cut) < len(wins)
            assert _differs(want, range_util.merged(windows, cut, c.keys)), (first, last, "no mask")
    if name.startswith("moved:"):
        assert wrapped >= 3, "the moved rings must wrap inside their ranges"
    if name == "p18":  # a bin's count passes a u16
        assert int(want.hist.max()) > 65_535
    # never-ingested keys and key 0 are among the queries
    assert (c.keys == 0).sum() == 1 and len(c.keys) == 300
