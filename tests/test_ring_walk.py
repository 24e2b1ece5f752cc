"""The moving-ring walk's inputs (tests/ring_util.py) can catch what they are
there for -- proved on the oracles alone, for every row of RING_ROWS:

  * after F every register of every window of the ring, for every service, is
    >= 1: every HLL lower bound can rise above zero before the ring moves;
  * in each window the advance exposes, T leaves at least 100 registers at a
    value a stale bound would have dropped: within 1 .. the minimum the
    retired window of the same slot held over the same sub-block of
    2^lb_shift registers;
  * G has ERROR spans of non-zero keys in every window about to retire (stale
    ERROR counts and slab partials exist), T has ERROR spans in every exposed
    window (they would show);
  * T has ends in retired windows and F in the window after the ring, which
    the sketch reference must never see (out-of-range accounting after a move).
"""
import numpy as np
import pytest

from geometry_util import RING_ROWS, expected_oor
from ring_util import reference, walk


def _errors_by_window(batch, cfg, nonzero_key=False):
    ok = ((batch.meta & np.uint32(0xFFFF)) < cfg.n_services) & ((batch.meta >> 19) & 3 == 2)
    if nonzero_key:
        ok &= batch.key_hash != 0
    return set((batch.end_ns[ok] // np.uint64(cfg.window_ns)).tolist())


@pytest.mark.parametrize("row", list(RING_ROWS))
def test_walk_inputs(row):
    wk, ref = walk(row), reference(row)
    cfg, w0, W, a = wk.cfg, wk.w0, wk.W, wk.a
    shift, lb_n = RING_ROWS[row]["lb"]
    assert lb_n > 0 and W & (W - 1) == 0

    # F raises every register of the ring
    for w, sk in ref["after_F"].items():
        assert sk is not None and int(sk[0].min()) >= 1, (w, "raise the row's fill")

    # T, in every exposed window, leaves registers below the retired bound
    retired, exposed = range(w0, w0 + a), range(w0 + W, w0 + W + a)
    for w in exposed:
        old = ref["after_G"][w - W][0].reshape(-1, 1 << shift).min(axis=1, keepdims=True)
        assert int(old.min()) >= 1
        new = ref["B"].windows[w][0].reshape(-1, 1 << shift)
        assert int(((new >= 1) & (new <= old)).sum()) >= 100, w

    # ERROR state in the slots about to retire, ERROR spans in the exposed windows
    assert set(retired) <= _errors_by_window(wk.batches["G"], cfg, nonzero_key=True)
    assert set(exposed) <= _errors_by_window(wk.batches["T"], cfg)
    for w in exposed:
        assert ref["B"].windows[w][1].any(), w

    # ends outside the ring of the moment, on both sides of the walk
    t_win = wk.batches["T"].end_ns // np.uint64(cfg.window_ns)
    assert int(((t_win >= w0) & (t_win < w0 + a)).sum()) > 0
    f_win = wk.batches["F"].end_ns // np.uint64(cfg.window_ns)
    assert int((f_win == w0 + W).sum()) > 0
    assert ref["A"].windows.keys() == set(range(w0, w0 + W))
    oor = [ref[c].stats["window_out_of_range"] for c in "ABCD"]
    assert 0 < oor[0] < oor[1] < oor[2] < oor[3]
    # half of T's first part (all of it on one window) ends in retired windows: far
    # more out of range than the 1 % make_batch strays
    assert expected_oor([wk.batches["T"]], cfg, w0 + a) > 0.2 * len(wk.batches["T"])
