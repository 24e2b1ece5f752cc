"""Every ingest path on a moving window ring, against the CPU oracle.

tests/test_gpu_geometry.py proves each kernel on a standing ring; here the
ring moves under load.  Each row of geometry_util.RING_ROWS (the three v2
small kernels, the ERROR table off, one window, the linear kernel, both small
exponential kernels, the exponential HBM path, the partitioned, atomic, binned
and dense paths) first asserts its geometry and then runs ring_util.run_walk:
a ring filled until every register and bound has risen, ERROR state left
unread in the slots about to retire, an advance by half the ring, a forced
reclaim, an advance by zero, a jump past the whole ring.  What
sa_window_advance must reset -- registers, HLL lower bounds, count-min cells,
ERROR slabs, per-slot ERROR counts -- would each show as a wrong register or
cell in the windows the advance exposes.

Modes:
  host    every batch through Engine.ingest
  device  columns copied once; every batch one ingest_device, alternating over
          two streams with no host synchronisation before an advance, a flush
          or a read: the engine's own ordering is under test
  graph   (Small rows) every batch but the fill as three ragged slices through
          ingest_device_many: both cached graphs are built before the advance
          and re-pointed (win_base, base_ns, base_slot) after it
"""
import pytest

from geometry_util import RING_ROWS, assert_geometry, config_of
from ring_util import DeviceFeed, run_walk, walk
from spanagg import Engine

pytestmark = pytest.mark.gpu

GRAPH_ROWS = ("ring_default", "ring_512", "ring_1024_noerr", "ring1", "ring_linear")
CASES = [(row, mode) for row in RING_ROWS for mode in ("host", "device", "graph")
         if mode != "graph" or row in GRAPH_ROWS]  # row-major: a row's modes share its reference
assert len(CASES) == 29


@pytest.mark.parametrize("row,mode", CASES, ids=[f"{r}-{m}" for r, m in CASES])
def test_ring_walk_vs_oracle(row, mode):
    wk = walk(row)
    with Engine(config_of(row)) as e:
        assert_geometry(e, row)
        if mode == "host":
            feed = lambda name: e.ingest(wk.batches[name])
        else:
            feed = DeviceFeed(e, wk, graph=mode == "graph")
        run_walk(e, row, feed)
