"""The kernels behind non-default engine geometries against the CPU oracle.

Every row of geometry_util.ROWS selects device code the rest of the suite runs
with a few thousand spans or not at all: the generic small-table kernels
(512 and 1,024 threads), the linear-threshold kernel, the generic exponential
kernel, the generic HBM and partitioned-scatter instances, the atomic path
chosen by the bucket count, the binned and dense paths with several services
and fewer than 17 buckets, and the config extremes (hll_p 4 .. 18, 65,536
services, count-min 1 x 2 and 8 x 64, one window, 1 and 63 buckets, tables of
256 .. 4,096 slots, the ERROR table on and off, unit s).

A row first asserts Engine.debug_geometry() against its expectation
(geometry_util works each out by hand), so it cannot slide onto another kernel
unnoticed.  It then ingests a thin batch (20,011 spans: at most one tile per
workgroup, a ragged tail) and a thick one (3,000,017 spans on small tables,
1,000,003 on HBM tables: several tiles per workgroup, more raised registers
than the deferred-raise queue holds, more ERROR (window, slot) pairs than the
LDS ERROR table holds) before one flush, and the thin batch again before a
second flush (the delta and the reset).  Bar: everything bit-exact, duration
sums within parity_util.SUM_RTOL.
"""
import zlib

import numpy as np
import pytest

from geometry_util import OFF, ROWS, THIN, assert_geometry, check_against_oracle, config_of, make_batch, ring_start
from spanagg import Engine

pytestmark = pytest.mark.gpu


def _rng(row):
    # dense5 takes binned5's batches: both must equal the same oracle, hence each other
    return np.random.default_rng(zlib.crc32({"dense5": "binned5"}.get(row, row).encode()))


def _engine(row):
    cfg = config_of(row)
    e = Engine(cfg)
    try:
        assert_geometry(e, row)
        e.window_advance(ring_start(cfg))
    except BaseException:
        e.close()
        raise
    return e, cfg, ring_start(cfg)


@pytest.mark.parametrize("row", list(ROWS))
def test_geometry_row_vs_oracle(row):
    r, rng = ROWS[row], _rng(row)
    e, cfg, w0 = _engine(row)
    with e:
        thin = make_batch(rng, THIN, cfg, r["n_keys"])
        thick = make_batch(rng, r["thick"], cfg, r["n_keys"])
        assert len(thick) >= 1_000_000
        e.ingest(thin)
        e.ingest(thick)
        check_against_oracle(e, [thin, thick], cfg, w0)
        e.ingest(thin)
        check_against_oracle(e, [thin], cfg, w0, earlier=[thin, thick])
        if r["lb"] == OFF:
            assert e.stats()["hll_filtered"] == 0


def test_hll_filter_on_a_one_window_ring():
    """Row ring1 (one window, one service, p = 10: one filter sub-block of all
    1,024 registers): 400,000 spans of distinct traces raise every register,
    so a second batch of fresh traces meets a lower bound above zero and the
    filter drops its low-rho updates -- with the registers still the oracle's.

    The second batch goes in as two launches.  A launch takes its bounds as
    the previous launch left them, and the wave that recomputes a sub-block's
    bound reads the registers while the launch's other raises may still be on
    their way (a stale read only lowers a lower bound), so a bound is only
    sure to cover earlier launches: the first launch may leave bound 0, the
    second then filters nothing and leaves at least the first launch's
    minimum, the third is the first that must filter."""
    r, rng = ROWS["ring1"], _rng("ring1 filter")
    e, cfg, w0 = _engine("ring1")
    with e:
        a = make_batch(rng, 400_000, cfg, r["n_keys"], distinct_traces=True)
        b = make_batch(rng, 400_000, cfg, r["n_keys"], distinct_traces=True)
        e.ingest(a)
        check_against_oracle(e, [a], cfg, w0)
        assert e.stats()["hll_filtered"] == 0
        e.ingest(b.slice(0, 200_000))
        e.ingest(b.slice(200_000, 400_000))
        check_against_oracle(e, [b], cfg, w0, earlier=[a])
        assert e.stats()["hll_filtered"] > 0


def test_every_span_an_error():
    """Row half17 with every span ERROR: each workgroup's 1,024-entry LDS ERROR
    table overflows at once (560 keys x 16 windows), and the count-min cells
    stay bit-exact."""
    r, rng = ROWS["half17"], _rng("half17 errors")
    e, cfg, w0 = _engine("half17")
    with e:
        b = make_batch(rng, 1_000_003, cfg, r["n_keys"], error_share=1.0)
        assert ((b.meta >> 19) & 3 == 2).all()
        e.ingest(b)
        check_against_oracle(e, [b], cfg, w0)
