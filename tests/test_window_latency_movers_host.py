"""sa_window_latency_movers without a GPU: the plain-Python rule
(spanagg.sketch.latency_movers) against the numpy restatement of
tests/latency_movers_util.py on the GPU tests' workloads, what those workloads
can tell apart, and the C-ABI's declarations.

The at-the-bound workload (65,536 services) is held against the restatement
on its used services only: its rows are the other cases' rule at a larger id.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import latency_movers_util as mu
import latency_util as lu
import spanagg
from spanagg import _lib, sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sketch_rows(c, call):
    B, Cr, k, ppm, mc, ms, fall = call
    hb = lu.ring_hists(c.ref, c.cfg, *B).sum(axis=0, dtype=np.uint64)
    hc = lu.ring_hists(c.ref, c.cfg, *Cr).sum(axis=0, dtype=np.uint64)
    return sketch.latency_movers(hb.tolist(), hc.tolist(), ppm, k, mc, ms, fall)


@pytest.mark.parametrize("name", mu.HOST_CASES)
def test_sketch_equals_the_restatement(name):
    c = mu.case(name)
    calls = c.calls if name != "long" else c.calls[::5]  # (the rule does not depend on a range's length)
    for call in calls:
        rows, n_eligible, n_matched = _sketch_rows(c, call)
        w = mu.want(c, call)
        assert rows == mu.items(w), (name, call[2:])
        assert (n_eligible, n_matched) == (w.n_eligible, w.n_matched), (name, call[2:])
        assert np.array_equal(w.q_ns_cur, lu.BIN_HI[w.q_bin_cur]) and np.array_equal(w.q_ns_base, lu.BIN_HI[w.q_bin_base])


def test_the_workloads_hit_their_targets():
    c = mu.case("crafted")
    rise, fall = mu.want(c, c.calls[0]), mu.want(c, c.calls[1])
    assert list(zip(rise.services.tolist(), rise.shift.tolist())) == mu.CRAFTED_RISE
    assert list(zip(fall.services.tolist(), fall.shift.tolist())) == mu.CRAFTED_FALL
    assert rise.n_eligible == 5 and rise.count_base.tolist() == [4, 4, 4]  # (service 3 has no baseline span)
    c = mu.case("ties")
    assert mu.want(c, (c.calls[0][0], c.calls[0][1], 12) + c.calls[0][3:]).services.tolist() == mu.TIES_ORDER
    c = mu.case("select")
    w = mu.want(c, c.calls[0])
    assert w.n_matched > mu.SELECT_K
    k = mu.SELECT_K
    assert (w.order_shift[k - 1], w.order_count[k - 1]) == (w.order_shift[k], w.order_count[k])  # the class straddles the cut


@pytest.mark.parametrize("wrong", mu.WRONG)
def test_every_known_mistake_shows_on_some_workload(wrong):
    seen = []
    for name in ("crafted", "ties", "ranges", "services64"):
        c = mu.case(name)
        for call in c.calls:
            right, bad = mu.want(c, call), mu.want(c, call, wrong)
            if mu.items(right) != mu.items(bad) or (right.n_eligible, right.n_matched) != (bad.n_eligible, bad.n_matched):
                seen.append((name, call[2:]))
    assert seen, wrong


def test_the_bound_workload():
    b = mu.bound_case()
    assert b.ids[0] == 0 and b.ids[-1] == mu.BOUND_S - 1 and len(b.ids) >= 200
    assert b.want.n_matched >= 20 and b.want.n_services == mu.BOUND_S


def test_declarations():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "spanagg.h")).read()
    for sym in ("sa_window_latency_movers", "sa_group_window_latency_movers", "sa_latency_movers_result_free"):
        assert hasattr(lib, sym) and re.search(r"\b%s\(" % sym, header), sym
    assert "#define SA_LATMOV_FALL 1u" in header and _lib.SA_LATMOV_FALL == spanagg.SA_LATMOV_FALL == 1
    # four u64, four u32, five u64, nine pointers
    assert C.sizeof(_lib.sa_latency_movers_result) == 4 * 8 + 4 * 4 + 5 * 8 + 9 * C.sizeof(C.c_void_p) == 160
    assert [f for f, _ in _lib.sa_latency_movers_result._fields_] == [
        "base_first", "base_last", "cur_first", "cur_last", "k", "n", "n_q", "flags", "n_services", "n_eligible",
        "n_matched", "spans_base", "spans_cur", "q_ppm", "services", "shift", "count_base", "count_cur", "q_bin_base",
        "q_bin_cur", "q_ns_base", "q_ns_cur"]
    assert "#define SA_OPT_ALL           0x7FFu" in header and "#define SA_ABI_VERSION 4" in header
    assert lib.sa_abi_version() == _lib.ABI_VERSION == 4
    assert {"LatencyMoversResult", "SA_LATMOV_FALL"} <= set(spanagg.__all__)
    out = C.POINTER(_lib.sa_latency_movers_result)()
    ppm = (C.c_uint32 * 1)(990_000)
    assert lib.sa_window_latency_movers(None, 0, 0, 0, 0, 1, 1, 1, ppm, 1, 0, C.byref(out)) == _lib.SA_EINVAL and not out
    assert lib.sa_group_window_latency_movers(None, 0, 0, 0, 0, 1, 1, 1, ppm, 1, 0, C.byref(out)) == _lib.SA_EINVAL
    lib.sa_latency_movers_result_free(None)
