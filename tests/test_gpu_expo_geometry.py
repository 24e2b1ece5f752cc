"""Exponential histograms across exp_max_size against the CPU oracle.

The counting pass (csrc/spanagg_expo.hip) changes shape with max_size: the
LDS entries of slab counting go from one per slot (2, 3, 5: no tail) to 15 at
4,096 (almost every series through tail records); an odd max_size leaves half
of an entry's last word unused; the fold bins go from 16 to 8 slots past
2,048, where a tail record's position needs its twelfth bit; the cached-probe
kernel's cache goes from 256 entries to 8.  Every row of
expo_geometry_util.ROWS (worked out by hand there) first asserts
Engine.debug_geometry() -- ingest kernel, counting kernel, entries, fold bins
-- and then runs one engine through

  1  a thin batch (20,011 spans), a thick one in one device launch
     (grid_max * 4,608 + 17 spans: more tail records per counting workgroup
     than its buffer's 4,096, and two heavy series that each overflow their
     fold bin's run of 64), a flush;
  2  launches A, B, C of narrow series far from 1 ms (every bucket index
     outside the index records' 14-bit field: the long route, at a settled
     scale >= 9), B moving half of them down 8 scales or more, a flush;
  3  the thin batch again (headers and scales reset), a flush, and an empty one.

The families of the workload (wide, narrow-far, field-edge, single, hot / cold)
are expo_geometry_util's; tests/test_expo_geometry_host.py shows on the CPU
that they reach these regimes.  Bar: parity_util._check (count, zero count,
scale, offset, every bucket, min and max exact; sums within 1e-9), the HLL
registers and count-min cells of every ring window bit-exact, no span dropped.

test_full_u16_counter fills one entry's u16 LDS counter to the workgroup span
limit (65,532) next to its word's other half.
"""
import numpy as np
import pytest

import pyoracle
from expo_geometry_util import (K_XT_CAP, ROWS, SLAB, assert_counting_geometry, config_of, plan_of, rng_of,
                                thick_size)
from geometry_util import check_against_oracle, ring_start
from spanagg import Config, Engine, pack_meta

pytestmark = pytest.mark.gpu
WG_SPANS = 65_532  # kMaxWgSpans: the spans of one counting workgroup


def _cus() -> int:
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _device_columns(batch):
    import torch
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(dev)
            for c in batch.columns()]
    torch.cuda.synchronize(dev)
    return cols


def _ingest_one_launch(e, batch):
    """A device-resident batch is one launch (a host batch goes in chunks of 2^20 spans)."""
    cols = _device_columns(batch)
    e.ingest_device(*cols)
    e.sync()


@pytest.mark.parametrize("row", list(ROWS))
def test_expo_geometry_row_vs_oracle(row):
    r, p, cfg, cus = ROWS[row], plan_of(row), config_of(row), _cus()
    w0 = ring_start(cfg)
    with Engine(cfg) as e:
        g = assert_counting_geometry(e, row, cus)
        e.window_advance(w0)
        thin = p.thin(rng_of(row, "thin"))
        thick = p.thick(rng_of(row, "thick"), thick_size(row, g["grid_max"], cus))
        if r["count"] == SLAB:
            assert len(thick) // g["grid_max"] > K_XT_CAP
        moving = p.moving(rng_of(row, "moving"))

        e.ingest(thin)
        _ingest_one_launch(e, thick)
        check_against_oracle(e, [thin, thick], cfg, w0)

        for b in moving:
            e.ingest(b)
        check_against_oracle(e, moving, cfg, w0, earlier=[thin, thick])

        e.ingest(thin)
        check_against_oracle(e, [thin], cfg, w0, earlier=[thin, thick] + moving)
        assert len(e.flush_exp().key_hash) == 0
        assert e.stats()["dropped_table_full"] == 0


def _same_word_pair(max_size=160):
    """(d_even, d_odd, index): two durations whose scale-20 bucket indices are
    index and index + 1 with index mod max_size even: positions 2q and 2q + 1
    of the circular bucket array, the two halves of one u32 word of u16 counts."""
    d = 3_000_000
    while True:
        i = pyoracle.expo_index(d / 1e6, 20)
        if i % max_size % 2 == 0:
            for d2 in range(d + 1, d + 8):
                if pyoracle.expo_index(d2 / 1e6, 20) == i + 1:
                    return d, d2, i
        d += 1


def test_full_u16_counter():
    """One series, grid_max * 65,532 spans in one launch: every counting
    workgroup adds 65,531 times to the low half of one LDS word and once to its
    high half (a carry would show in the neighbour bucket).  The same batch
    twice (the second launch counts with the entry the first one selected),
    then, in a second interval, four spans more: the engine splits the batch
    above the limit.  The expectation is analytic and exact."""
    import torch
    dev = torch.device("cuda", 0)
    M, key = 160, 0x5EED0FAC0DE
    d_even, d_odd, ix = _same_word_pair(M)
    q, pos = divmod(ix % M, 2)
    assert pos == 0 and (ix + 1) % M == 2 * q + 1  # at the final scale, 20: two adjacent buckets
    cfg = Config(exp_max_size=M, n_services=1, n_windows=16)
    with Engine(cfg) as e:
        g = e.debug_geometry()
        assert (g["path"], g["kernel"], g["expo_count"]) == ("ExpoSmall", "expo_specialised", SLAB), g
        assert g["expo_entries"] > 0
        G = g["grid_max"]
        n, extra = G * WG_SPANS, 4
        w0 = ring_start(cfg)
        e.window_advance(w0)
        end_ns = w0 * cfg.window_ns + 5
        kcol = torch.full((n + extra,), key, dtype=torch.int64, device=dev)
        end = torch.full((n + extra,), end_ns, dtype=torch.int64, device=dev)
        start = torch.full((n + extra,), end_ns - d_even, dtype=torch.int64, device=dev)
        start[WG_SPANS - 1:n:WG_SPANS] = end_ns - d_odd  # the last span of every workgroup's share
        t0 = torch.arange(n + extra, dtype=torch.int64, device=dev)
        t1 = torch.full((n + extra,), 7, dtype=torch.int64, device=dev)
        meta = torch.full((n + extra,), int(pack_meta(0, 2, 0)), dtype=torch.int32, device=dev)
        torch.cuda.synchronize(dev)
        cols = (kcol, start, end, t0, t1, meta)

        def expect(res, spans, odd):
            assert [int(k) for k in res.key_hash] == [key]
            assert (int(res.count[0]), int(res.zero_count[0])) == (spans, 0)
            assert (int(res.scale[0]), int(res.offset[0])) == (20, ix)
            assert [int(c) for c in res.buckets[0]] == [spans - odd, odd]
            assert int(res.sum_ns[0]) == (spans - odd) * d_even + odd * d_odd
            assert (res.min[0], res.max[0]) == (d_even / 1e6, d_odd / 1e6)
            assert res.sum[0] == int(res.sum_ns[0]) / 1e6

        e.ingest_device(*cols, n=n)
        e.ingest_device(*cols, n=n)
        expect(e.flush_exp(), 2 * n, 2 * G)
        e.ingest_device(*cols, n=n + extra)
        expect(e.flush_exp(), n + extra, G)
        assert e.stats()["dropped_table_full"] == 0
