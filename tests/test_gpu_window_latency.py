"""sa_window_latency on the GPU (SA_OPT_WINDOW_LATENCY, spanagg_latency.hip)
against the numpy reference of tests/latency_util.py; every comparison is ==.

  the ring walk   all 29 (row, mode) cases of tests/test_gpu_ring.py with the
                  option on: ring_util.run_walk unchanged -- RED, registers,
                  cells and stats still equal the oracle -- and after batches
                  L2, T, U and V every window's histograms against the
                  reference (retired slots cleared, the jump past the ring,
                  host / two-stream / ingest_device_many feeds, every table path)
  service counts  1, 64, 128, 129 and 1,000 services (both sides of the LDS
                  bound, the HBM form), a batch in drawn order (several
                  passes over a range: its spans lie in all eight windows)
                  and sorted by end (one pass, everything in LDS)
  hot cell        100,000 spans on one service, bin and window
  widths          1, 2, W - 1, W on a moved 32-window ring: every output equals
                  the range query over its own span
  selections, the crafted rank rows, n_q = 8, idempotence, a query behind an
  unsynchronised device ingest, every error return, groups of three and of
  one member over both transports.
"""
import ctypes as C
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import latency_util as lu
from geometry_util import assert_geometry, config_of, make_batch, ring_start
from ring_util import DeviceFeed, run_walk, walk
from spanagg import LAT_MAX_Q, Config, Engine, Group, SpanAggError, SpanBatch, _lib, pack_meta, sketch
from spanagg._lib import OPT_GROUP_COPY, OPT_GROUP_RCCL, OPT_WINDOW_LATENCY
from test_gpu_ring import CASES

pytestmark = pytest.mark.gpu

Q3 = (0.5, 0.95, 0.99)
CHECKED = ("L2", "T", "U", "V")  # (not G: the walk wants nothing to join there)
FED = ("F", "L2", "G", "T", "U", "V")


def with_latency(cfg) -> Config:
    return dataclasses.replace(cfg, options=cfg.options | OPT_WINDOW_LATENCY)


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


@functools.lru_cache(maxsize=2)
def walk_reference(row):
    """After each checked batch of the row's walk: what window_latency_series
    over the whole ring (width 1, hist) must return."""
    wk = walk(row)
    want = {}
    for i, name in enumerate(FED):
        if name in CHECKED:
            steps = [(wk.base[n], wk.batches[n]) for n in FED[:i + 1]]
            base = wk.base[name]
            want[name] = lu.expected(lu.window_hists(wk.cfg, steps), wk.cfg, base, base + wk.W - 1, 1, None, Q3)
    return want


@pytest.mark.parametrize("row,mode", CASES, ids=[f"{r}-{m}" for r, m in CASES])
def test_ring_walk_with_latency(row, mode):
    wk, want = walk(row), walk_reference(row)
    assert len(CASES) == 29
    with Engine(with_latency(config_of(row))) as e:
        assert_geometry(e, row)
        host = lambda name: e.ingest(wk.batches[name])
        inner = host if mode == "host" else DeviceFeed(e, wk, graph=mode == "graph")

        def feed(name):
            inner(name)
            if name in CHECKED:
                base = wk.base[name]
                lu.assert_latency(e.window_latency_series(base, base + wk.W - 1, 1, hist=True), want[name], name)

        run_walk(e, row, feed)
        # the walk's last reads and flush cleared nothing
        base = wk.base["V"]
        lu.assert_latency(e.window_latency_series(base, base + wk.W - 1, 1, hist=True), want["V"], "end")


def _svc_cfg(S, W=8) -> Config:
    return Config(n_services=S, n_windows=W, hll_p=10, key_capacity=1000, options=OPT_WINDOW_LATENCY)


@functools.lru_cache(maxsize=2)
def svc_case(S):
    cfg = _svc_cfg(S)
    w0 = ring_start(cfg)
    batch = make_batch(np.random.default_rng(zlib.crc32(b"latency_svc") + S), 200_000, cfg, 500, w0=w0)
    return SimpleNamespace(cfg=cfg, w0=w0, batch=batch, ref=lu.window_hists(cfg, [(w0, batch)]))


@pytest.mark.parametrize("order", ["drawn", "sorted"])
@pytest.mark.parametrize("S", [1, 64, 128, 129, 1000])
def test_service_counts(S, order):
    c = svc_case(S)
    b, W = c.batch, c.cfg.n_windows
    if order == "sorted":
        by_end = np.argsort(b.end_ns, kind="stable")
        b = SpanBatch(*[col[by_end] for col in b.columns()])
    with Engine(c.cfg) as e:
        e.window_advance(c.w0)
        e.ingest(b)
        last = c.w0 + W - 1
        lu.assert_latency(e.window_latency_series(c.w0, last, 1, hist=True),
                          lu.expected(c.ref, c.cfg, c.w0, last, 1, None, Q3))
        r = e.window_latency(c.w0, last, hist=S <= 129)
        lu.assert_latency(r, lu.expected(c.ref, c.cfg, last, last, W, None, Q3))
        st = e.stats()
        assert int(r.count.sum()) == st["spans"] - st["invalid_service"] - st["window_out_of_range"]


@pytest.mark.parametrize("S,W", [(128, 16), (64, 32), (100, 64)])
def test_more_windows_than_the_passes_hold(S, W):
    """One, two and one ring slots fit in LDS: eight passes hold 8, 16 and 8
    of the 16, 32 and 64 windows a drawn batch lies in, and the last pass sends
    the spans of the others straight to the ring."""
    cfg = _svc_cfg(S, W)
    w0 = ring_start(cfg)
    batch = make_batch(np.random.default_rng(zlib.crc32(b"latency_passes") + S), 150_000, cfg, 500, w0=w0)
    ref = lu.window_hists(cfg, [(w0, batch)])
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(batch)
        last = w0 + W - 1
        lu.assert_latency(e.window_latency_series(w0, last, 1, hist=True), lu.expected(ref, cfg, w0, last, 1, None, Q3))
        assert int(e.window_latency(w0, last).count.sum()) == int(lu.ring_hists(ref, cfg, w0, last).sum())


def test_range_that_starts_outside_the_ring():
    """The first 6,000 spans end before the ring, so the second workgroup's
    range (3,884 spans each) starts with 2,116 of them: the home slot is the
    first in-ring span's wherever it lies in the range; and a batch with no
    in-ring span at all counts nothing."""
    cfg = _svc_cfg(6)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"latency_outside"))
    inside = make_batch(rng, 60_000, cfg, 500, w0=w0)
    before = make_batch(rng, 6_000, cfg, 500, w0=w0 - 2 * cfg.n_windows)
    batch = SpanBatch(*[np.concatenate(c) for c in zip(before.columns(), inside.columns())])
    ref = lu.window_hists(cfg, [(w0, batch)])
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(before)
        last = w0 + cfg.n_windows - 1
        assert not e.window_latency_series(w0, last, 1).count.any()
        e.ingest(inside)
        e.ingest(before)
        lu.assert_latency(e.window_latency_series(w0, last, 1, hist=True), lu.expected(ref, cfg, w0, last, 1, None, Q3))
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(batch)
        lu.assert_latency(e.window_latency_series(w0, last, 1, hist=True), lu.expected(ref, cfg, w0, last, 1, None, Q3))


def test_hot_cell():
    """One LDS word and one ring word take every add."""
    cfg, n = _svc_cfg(4), 100_000
    w0 = ring_start(cfg)
    end = np.full(n, (w0 + 3) * cfg.window_ns + 17, dtype=np.uint64)
    k = np.arange(1, n + 1, dtype=np.uint64)
    batch = SpanBatch(k, end - np.uint64(5_000_000), end, k, k, pack_meta(np.full(n, 2), np.zeros(n), np.zeros(n)))
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(batch)
        r = e.window_latency_series(w0, w0 + cfg.n_windows - 1, 1, hist=True)
        want = np.zeros((cfg.n_windows, 4, 256), np.uint64)
        want[3, 2, sketch.latency_bin(5_000_000)] = n
        assert np.array_equal(r.hist, want)
        assert int(r.count[3, 2]) == n and int(r.count.sum()) == n
        assert (r.q_bin[3, 2] == sketch.latency_bin(5_000_000)).all()


@functools.lru_cache(maxsize=1)
def moved_case():
    """ring_1024_noerr's 32 windows, moved by 13: the resident windows wrap the slots."""
    cfg = with_latency(config_of("ring_1024_noerr"))
    rng = np.random.default_rng(zlib.crc32(b"latency_moved"))
    w0 = ring_start(cfg)
    base = w0 + 13
    steps = [(w0, make_batch(rng, 60_000, cfg, 700, w0=w0)), (base, make_batch(rng, 60_000, cfg, 700, w0=base))]
    return SimpleNamespace(cfg=cfg, steps=steps, base=base, ref=lu.window_hists(cfg, steps))


def _loaded(c, cls=Engine, *a):
    x = cls(*a, c.cfg) if a else cls(c.cfg)
    for base, batch in c.steps:
        x.window_advance(base)
        x.ingest(batch)
    return x


def _same(a, b):
    for f in ("services", "q_ppm", "count", "q_bin", "q_ns"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert (a.hist is None) == (b.hist is None) and (a.hist is None or np.array_equal(a.hist, b.hist))


def test_widths_on_a_moved_ring():
    c = moved_case()
    W, base = c.cfg.n_windows, c.base
    with _loaded(c) as e:
        for width in (1, 2, W - 1, W):
            first, last = base + width - 1, base + W - 1
            r = e.window_latency_series(first, last, width, hist=True)
            lu.assert_latency(r, lu.expected(c.ref, c.cfg, first, last, width, None, Q3), width)
            for o, t in enumerate(range(first, last + 1)):
                one = e.window_latency(t - width + 1, t, hist=True)
                for f in ("count", "q_bin", "q_ns", "hist"):
                    assert np.array_equal(getattr(one, f)[0], getattr(r, f)[o]), (width, t, f)


def test_selections_quantiles_and_idempotence():
    cfg = with_latency(config_of("ring_512"))  # 2 services, 4 windows
    cfg = dataclasses.replace(cfg, n_services=12)
    rng = np.random.default_rng(zlib.crc32(b"latency_sel"))
    w0 = ring_start(cfg)
    steps = [(w0, make_batch(rng, 50_000, cfg, 500, w0=w0)), (w0, lu.crafted_batch(cfg, w0 + 1))]
    ref = lu.window_hists(cfg, steps)
    q8 = (1e-6, 0.1, 0.25, 0.5, 0.75, 0.9, 0.999, 1.0)
    assert len(q8) == LAT_MAX_Q
    with Engine(cfg) as e:
        e.window_advance(w0)
        for _, b in steps:
            e.ingest(b)
        last = w0 + cfg.n_windows - 1
        sel = (7, 2, 11, 0)
        r = e.window_latency_series(w0 + 1, last, 2, services=sel, quantiles=q8, hist=True)
        assert r.services.tolist() == list(sel) and r.q_ppm.tolist() == lu.ppm_of(q8)
        assert (r.first, r.last, r.width) == (w0 + 1, last, 2)
        lu.assert_latency(r, lu.expected(ref, cfg, w0 + 1, last, 2, sel, q8))
        _same(r, e.window_latency_series(w0 + 1, last, 2, services=sel, quantiles=q8, hist=True))
        no_hist = e.window_latency_series(w0 + 1, last, 2, services=sel, quantiles=q8)
        assert no_hist.hist is None and np.array_equal(no_hist.q_ns, r.q_ns)


def test_crafted_rank_rows():
    cfg = _svc_cfg(3, W=2)
    w0 = ring_start(cfg)
    q = [p / 1e6 for p in lu.CRAFTED_PPM]
    with Engine(cfg) as e:
        e.window_advance(w0)
        e.ingest(lu.crafted_batch(cfg, w0 + 1))
        r = e.window_latency(w0 + 1, w0 + 1, quantiles=q, hist=True)
        assert r.q_ppm.tolist() == list(lu.CRAFTED_PPM)
        assert r.count[0].tolist() == [3, 1, 0]
        assert r.q_bin[0, 0].tolist() == list(lu.CRAFTED_WANT)          # three spans in bins a < b < c
        assert r.q_bin[0, 1].tolist() == [200] * 6                      # a row with one span
        assert not r.q_bin[0, 2].any() and not r.q_ns[0, 2].any()       # an empty row
        assert r.q_ns[0, 0].tolist() == [sketch.latency_bin_bounds(b)[1] for b in lu.CRAFTED_WANT]
        assert r.q_ns[0, 1].tolist() == [sketch.latency_bin_bounds(200)[1]] * 6
        assert r.hist[0, 0].nonzero()[0].tolist() == list(lu.CRAFTED_BINS)
        empty = e.window_latency(w0, w0, quantiles=q)
        assert not empty.count.any() and not empty.q_bin.any() and not empty.q_ns.any()


def test_query_behind_an_unsynchronised_device_ingest():
    c = moved_case()
    (b0, first_batch), (base, batch) = c.steps
    W = c.cfg.n_windows
    with Engine(c.cfg) as e:
        e.window_advance(b0)
        e.ingest(first_batch)
        e.window_advance(base)
        feed = DeviceFeed(e, SimpleNamespace(batches={"F": batch}, row="window_latency"))
        feed("F")  # on a stream of its own; nothing waits for it
        r = e.window_latency_series(base, base + W - 1, 1, hist=True)
        lu.assert_latency(r, lu.expected(c.ref, c.cfg, base, base + W - 1, 1, None, Q3))
        _same(r, e.window_latency_series(base, base + W - 1, 1, hist=True))


def test_errors_leave_the_engine_usable():
    c = moved_case()
    W, S, first, last = c.cfg.n_windows, c.cfg.n_services, c.base, c.base + c.cfg.n_windows - 1
    want = lu.expected(c.ref, c.cfg, first, last, 1, None, Q3)
    with _loaded(c) as e:
        ok = lambda: lu.assert_latency(e.window_latency_series(first, last, 1, hist=True), want)
        out = C.POINTER(_lib.sa_latency_result)()
        ids, two, ppm = (C.c_uint32 * 2)(0, 0), (C.c_uint32 * 2)(0, S), (C.c_uint32 * 9)(*([500_000] * 9))
        zero, big = (C.c_uint32 * 1)(0), (C.c_uint32 * 1)(1_000_001)
        call = lambda sv, n, q, nq, flags, o=out: e.lib.sa_window_latency(
            e._h, first, last, 1, sv, n, q, nq, flags, C.byref(o) if o is not None else None)
        bad = [(None, 1, ppm, 1, 0),        # services == NULL with n_sel != 0
               (ids, 0, ppm, 1, 0),         # and the reverse
               (two, 2, ppm, 1, 0),         # an id >= n_services
               (ids, 2, ppm, 1, 0),         # a repeated id
               (None, 0, ppm, 0, 0), (None, 0, ppm, 9, 0),   # n_q of 0 or above 8
               (None, 0, zero, 1, 0), (None, 0, big, 1, 0),  # a q_ppm outside 1..10^6
               (None, 0, ppm, 1, 2)]        # unknown flag bits
        for args in bad:
            assert call(*args) == _lib.SA_EINVAL and not out, args[1:]
            ok()
        assert call(None, 0, ppm, 1, 0, None) == _lib.SA_EINVAL  # a null `out`
        for a, b, width in ((first + 1, first, 1), (first, last, 0), (last, last, W + 1), (first, last, 2),
                            (first - 1, last, 1), (first, last + 1, 1), (0, 0, 2)):
            _raises(_lib.SA_ERANGE, lambda: e.window_latency_series(a, b, width))
            ok()
        assert call(None, 0, ppm, 8, 1) == _lib.SA_OK and out and out.contents.n_q == 8 and out.contents.hist
        e.lib.sa_latency_result_free(out)
    with Engine(dataclasses.replace(c.cfg, options=0)) as e:  # without the option
        e.window_advance(c.base)
        _raises(_lib.SA_ESTATE, lambda: e.window_latency(first, last))
        assert e.stats()["window_base"] == c.base


def test_result_size_limits_and_create_limits():
    """n_out * n_sel > 2^16 with SA_LAT_HIST; the ring's 2^18 rows at create."""
    cfg = Config(n_services=4097, n_windows=16, hll_p=4, key_capacity=1000, options=OPT_WINDOW_LATENCY)
    w0 = ring_start(cfg)
    with Engine(cfg) as e:
        e.window_advance(w0)
        _raises(_lib.SA_EINVAL, lambda: e.window_latency_series(w0, w0 + 15, 1, hist=True))  # 16 * 4,097 rows
        r = e.window_latency_series(w0, w0 + 15, 1)
        assert r.count.shape == (16, 4097) and not r.count.any()
        assert e.window_latency_series(w0, w0 + 14, 1, hist=True).hist.shape == (15, 4097, 256)
    for W, S in ((4096, 65), (8, 32769)):  # 2^18 + 2^12 and 2^18 + 8 rows
        with pytest.raises(SpanAggError) as x:
            Engine(Config(n_services=S, n_windows=W, hll_p=4, options=OPT_WINDOW_LATENCY))
        assert x.value.code == _lib.SA_EINVAL


@pytest.mark.parametrize("devices,option,rccl", [([0, 0, 0], OPT_GROUP_COPY, False), ([0, 0, 0], OPT_GROUP_RCCL, False),
                                                 ([0], OPT_GROUP_COPY, False), ([0], OPT_GROUP_RCCL, True)])
def test_group_equals_one_engine(devices, option, rccl):
    """Members on device 0 (a communicator cannot hold two of them: those
    groups merge through device copies whatever they ask for); a group of one
    that asks for RCCL all-reduces for real."""
    c = moved_case()
    W, first, last = c.cfg.n_windows, c.base, c.base + c.cfg.n_windows - 1
    gcfg = dataclasses.replace(c.cfg, options=c.cfg.options | option)
    with _loaded(SimpleNamespace(cfg=gcfg, steps=c.steps), Group, devices) as g, _loaded(c) as e:
        assert g.size == len(devices) and g.uses_rccl == rccl
        for a, b, width, sel in ((first, last, 1, None), (first + 4, last, 5, (0,)), (last, last, W, None)):
            rg = g.window_latency_series(a, b, width, services=sel, hist=True)
            lu.assert_latency(rg, lu.expected(c.ref, c.cfg, a, b, width, sel, Q3), (a - first, width))
            _same(rg, e.window_latency_series(a, b, width, services=sel, hist=True))
        _same(g.window_latency(first + 1, last - 1), e.window_latency(first + 1, last - 1))
        _raises(_lib.SA_ERANGE, lambda: g.window_latency(first - 1, last))
        _raises(_lib.SA_EINVAL, lambda: g.window_latency(first, last, services=(0, 0)))
        _raises(_lib.SA_EINVAL, lambda: g.window_latency(first, last, quantiles=(0.0,)))
        _same(g.window_latency(first, last), e.window_latency(first, last))
    with Group([0, 0], dataclasses.replace(gcfg, options=option)) as g:  # without the option
        _raises(_lib.SA_ESTATE, lambda: g.window_latency(first, last))
