"""HLL registers at every rho on every ingest path, against the CPU oracle.

The rest of the GPU suite feeds the HyperLogLog side random trace ids: no rho
above the high twenties, lower bounds of 0 to 3.  Here the ids come from
tests/hll_util.py's families -- xxh64 run backwards -- so each of the six
pieces of device code that turn a trace id into (register, rho) meets every
rho 1 .. 65 - p in three bit patterns, the hand-over between the 32-bit halves
of x << p, the sentinel bit alone, lanes of one wave raising one word, and a
lower-bound filter loaded to 20 with single registers left at 1 where its
reduction could overlook them.  tests/test_hll_ids_host.py proves on the CPU
that the batches are what they claim.

Rows: every row of geometry_util.RING_ROWS (the linear-threshold kernel, the
v2 kernel's plain and lean forms, both small exponential kernels, the HBM
kernel behind ExpoHbm and Atomic, the partitioned scatter, the binned and
dense scatter) and hll_util.HLL_ROWS (hll_p 4 and 18 on the lean, plain and
binned forms).  Every test asserts its geometry first and compares through
geometry_util.check_against_oracle: registers, count-min cells, RED rows and
stats bit-exact (duration sums by parity_util.SUM_RTOL).

The filter: hll_filtered may count only spans whose rho did not exceed their
register's value when their launch began (hll_util.CannotRaise counts those,
launch by launch); on the kernels that filter (hll_util.FILTER_ROWS) it must
have moved by the end, on the others -- no filter geometry at p = 4, or a
kernel that does not read the bounds (ring_util.FILTERS) -- it stays 0.
"""
import functools
import zlib

import numpy as np
import pytest

import hll_util as hu
import pyoracle
import range_util
import series_util
from geometry_util import assert_geometry, check_against_oracle, key_pool, ring_start, unit_div
from hll_util import ALL_ROWS, FILTER_ROWS, FLOOR, HLL_ROWS, OFF, Ring, config_of
from parity_util import assert_red_equal
from ring_util import in_ring, slices
from spanagg import Engine

pytestmark = pytest.mark.gpu

DEVICE_ROWS = ("ring_default", "ring_expo_spec", "ring_binned")
CASES = [(row, "host") for row in ALL_ROWS] + [(row, m) for row in DEVICE_ROWS for m in ("device", "many")]


def _engine(row):
    cfg = config_of(row)
    e = Engine(cfg)
    try:
        g = assert_geometry(e, row, HLL_ROWS)
        e.window_advance(ring_start(cfg))
    except BaseException:
        e.close()
        raise
    return e, cfg, ring_start(cfg), g


@functools.lru_cache(maxsize=4)
def _mixed(row, touch_zero):
    cfg = config_of(row)
    return hu.mixed(cfg, ring_start(cfg), ALL_ROWS[row]["n_keys"], touch_zero)


def _on_device(batch):
    import torch
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(np.ascontiguousarray(c).view(np.int64 if c.dtype == np.uint64 else np.int32)).to(dev)
            for c in batch.columns()]
    torch.cuda.synchronize(dev)
    return cols


def _ingest(e, batch, mode, keep):
    """host: Engine.ingest; device: one ingest_device; many: three ragged
    slices at even offsets through ingest_device_many.  keep: the device
    columns, alive until the caller has flushed."""
    if mode == "host":
        return e.ingest(batch)
    cols = _on_device(batch)
    keep.append(cols)
    if mode == "device":
        e.ingest_device(*cols)
    else:
        cuts = slices(len(batch), 3, np.random.default_rng(zlib.crc32(b"many")))
        e.ingest_device_many([tuple(c[a:b] for c in cols) for a, b in cuts])


def _slot_order(e, ring):
    """The ring's registers by position in the engine's array."""
    return np.concatenate([e.window_read(ring.w0 + ((s - ring.w0) & (ring.W - 1))).hll.ravel() for s in range(ring.W)])


@pytest.mark.parametrize("row,mode", CASES, ids=[f"{r}-{m}" for r, m in CASES])
def test_every_rho(row, mode):
    """every_rho + half_boundary + shared_word shuffled into random traffic,
    then the crafted spans alone once more.  host: position 0 is raised to
    65 - p by a crafted span; device, many: no span lands on it at all."""
    touch_zero = mode == "host"
    batch, alone, claims = _mixed(row, touch_zero)
    e, cfg, w0, _ = _engine(row)
    ring, keep = Ring(cfg, w0), []
    with e:
        _ingest(e, batch, mode, keep)
        check_against_oracle(e, [batch], cfg, w0)
        want = hu.expected_registers(ring, claims)
        high = {w: v > 30 for w, v in want.items()}  # (beyond random traffic: the crafted value stands)
        for w in want:
            got = e.window_read(w).hll
            assert np.array_equal(got[high[w]], want[w][high[w]]) and (got >= want[w]).all(), w
        assert _slot_order(e, ring)[0] == (ring.top if touch_zero else 0)
        _ingest(e, alone, mode, keep)  # registers are idempotent, counts add up
        check_against_oracle(e, [alone], cfg, w0, earlier=[batch])
        assert _slot_order(e, ring)[0] == (ring.top if touch_zero else 0)
        if row not in FILTER_ROWS:
            assert e.stats()["hll_filtered"] == 0


@pytest.mark.parametrize("row", ["ring_default", "ring_1024_noerr", "ring_binned", "ring_part"])
def test_register_zero_untouched(row):
    """Spans that may not reach a sketch (service out of range, end outside the
    ring), each with an id of index 0 and rho 64 - p or 65 - p: the lanes that
    have nothing to do read position 0 and must leave it, and every other
    register, at 0."""
    e, cfg, w0, _ = _engine(row)
    with e:
        b = hu.invalid_spans(cfg, w0, ALL_ROWS[row]["n_keys"])
        e.ingest(b)
        check_against_oracle(e, [b], cfg, w0)
        assert not _slot_order(e, Ring(cfg, w0)).any()
        st = e.stats()
        assert st["hll_filtered"] == 0 and st["invalid_service"] + st["window_out_of_range"] == len(b)


def _load_floor(e, row, cfg, w0, g, probes=True):
    """filter_floor's batches, one launch each: the floor, the top-up in as
    many launches as visit every sub-block, then (probes) the probe twice.
    Checks the oracle and the filter's bound after each step; returns the
    batches ingested and the filter_floor namespace."""
    geo = hu.filter_geometry(row)
    filters = hu.filters(row)
    if hu.row_of(row)["lb"] != OFF:
        assert (g["lb_shift"], g["lb_n"]) == geo
    else:
        assert g["lb_n"] == 0
    ff = hu.filter_floor(cfg, w0, hu.row_of(row)["n_keys"], geo, partial=row == hu.DEEP)
    tops = hu.equal_slices(ff.topup, hu.topup_launches(geo[1], g["block"]))
    cr, done = hu.CannotRaise(cfg, w0), []
    ring = ff.ring
    steps = [[ff.floor], tops + [ff.probe], [ff.probe]] if probes else [[ff.floor], tops]
    for k, step in enumerate(steps):
        for b in step:
            assert 0 < len(b) <= min(1 << 20, g["grid_max"] * 65_520)  # one launch (csrc/engine_ingest.cpp)
            e.ingest(b)
            cr.launch(b)
            n = e.stats()["hll_filtered"]
            assert n <= cr.count if filters else n == 0, (k, n, cr.count)
        check_against_oracle(e, step, cfg, w0, earlier=done)
        done += step
        n = e.stats()["hll_filtered"]
        assert n <= cr.count if filters else n == 0, (k, n, cr.count)
        got = _slot_order(e, ring)
        assert np.array_equal(got, cr.state), k
        if k == 0:
            in_floor = np.isin(np.arange(ring.regs) >> geo[0], ff.floored)
            in_floor[ff.low] = False
            assert (got[ff.low] == 1).all() and (got[in_floor] == FLOOR).all()
        if probes and k >= 1:
            assert (got[ff.low] == 2).all() and (got[ff.up] == FLOOR + 1).all(), k
    if filters:
        assert e.stats()["hll_filtered"] > 0
    return done, ff


@pytest.mark.parametrize("row", list(ALL_ROWS) + [hu.DEEP])
def test_filter_floor(row):
    """Every register at 20 but single ones at 1 -- at the first and last byte
    of a 16-byte quad, in the last quad of a lane's pass, at the sub-block's
    end -- then, once every sub-block's bound has been refreshed, rho 19, 20,
    21 into every sub-block and rho 2 into the low registers: a bound that
    overlooked a low register would swallow the 2, a bound one too high the 21.
    The last row (hll_util.DEEP) has sub-blocks of 512 quads: low registers also
    in the last quad of the two-phase bound's first pass and the first of its
    second loop."""
    e, cfg, w0, g = _engine(row)
    with e:
        _load_floor(e, row, cfg, w0, g)


@pytest.mark.parametrize("row", ["ring_default", "ring_binned", "ring1"])
def test_filter_after_advance(row):
    """With the bounds at 20, the ring moves by two ring lengths: every slot is
    cleared and reused.  rho 1 and rho 2 on every register of a few sub-blocks
    must all register -- a bound that survived the clear would swallow them."""
    e, cfg, w0, g = _engine(row)
    with e:
        _load_floor(e, row, cfg, w0, g, probes=False)
        before = e.stats()
        assert before["hll_filtered"] > 0
        w1 = w0 + 2 * cfg.n_windows
        e.window_advance(w1)
        ring = Ring(cfg, w1)
        assert not _slot_order(e, ring).any()
        b, claims = hu.after_advance_spans(cfg, w1, ALL_ROWS[row]["n_keys"], hu.filter_geometry(row))
        e.ingest(b)
        o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
        o.ingest(b)
        assert_red_equal(e.flush(), o.series(), unit_div=unit_div(cfg))
        want, seen = hu.expected_registers(ring, claims), set(o.window_ids())
        for w in range(w1, w1 + ring.W):
            sk = e.window_read(w)
            assert np.array_equal(sk.hll, want[w]), w
            if w in seen:
                assert np.array_equal(sk.hll, o.window(w)[0]) and np.array_equal(sk.cms, o.window(w)[1]), w
            else:
                assert not sk.cms.any() and not want[w].any(), w
        st = e.stats()
        assert st["hll_filtered"] == before["hll_filtered"]  # every span raised a cleared register
        assert st["spans"] == before["spans"] + len(b)
        assert st["window_out_of_range"] == before["window_out_of_range"]


@pytest.mark.parametrize("row", ["p4_plain", "ring_default"])
def test_range_and_series_at_high_rho(row):
    """window_range and window_series over the ring every_rho left: histogram
    bins up to 65 - p (61 at p = 4, of SA_HLL_HIST_BINS = 64) are populated,
    and the estimates are those of the oracle's histograms, bit for bit."""
    from spanagg import hll_estimate_hist
    batch, _, claims = _mixed(row, True)
    e, cfg, w0, _ = _engine(row)
    W, top = cfg.n_windows, 65 - cfg.hll_p
    # the values the crafted registers keep in the merge (a window's register can hide the other window's)
    crafted = np.maximum.reduce(list(hu.expected_registers(Ring(cfg, w0), claims).values()))
    held = sorted(int(v) for v in set(crafted.ravel()) if v > 30)
    assert top in held and len(held) >= (top - 30) // 2
    with e:
        e.ingest(batch)
        o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
        o.ingest(in_ring(batch, cfg, w0))
        windows = {w: o.window(w) for w in range(w0, w0 + W)}
        n_keys = ALL_ROWS[row]["n_keys"]
        keys = range_util.query_keys(key_pool(n_keys), n_keys)
        r = e.window_range(w0, w0 + W - 1, keys, registers=True, cells=True)
        want = range_util.merged(windows, range(w0, w0 + W), keys)
        range_util.assert_range_equal(r, want, cfg, row)
        assert (want.hist[:, held].sum(axis=0) > 0).all() and not want.hist[:, top + 1:].any()
        assert [float(d) for d in r.distinct] == [hll_estimate_hist(h, cfg.hll_p) for h in want.hist]
        s = e.window_series(w0 + 1, w0 + W - 1, width=2, keys=keys)
        ws = series_util.series(windows, w0 + 1, w0 + W - 1, 2, keys)
        series_util.assert_series_equal(s, ws, cfg, w0 + 1, w0 + W - 1, 2, row)
        assert np.array_equal(ws.hist[-1], want.hist)  # (two windows: the last output spans the ring)
        assert [float(d) for d in s.distinct[-1]] == [hll_estimate_hist(h, cfg.hll_p) for h in ws.hist[-1]]
