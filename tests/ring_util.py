"""The moving window ring: one walk per row of geometry_util.RING_ROWS.

sa_window_advance recycles ring slots while the engine carries per-slot state
from launch to launch.  For every retired slot it clears the HLL registers,
the HLL lower bounds of the slot's sub-blocks, the count-min cells, the
per-workgroup ERROR slabs and the exact per-slot ERROR counts, ordered after
the launches in flight and before every later one.  The walk loads a ring until
each of those holds something, moves it, and compares with oracles that never
saw a ring:

  F    max(fill x regs, 200,000) spans of distinct traces over the ring at w0
       (regs = n_windows x n_services x 2^hll_p; fill = 24 unless the row says
       more): every register of the ring ends >= 1, so every lower bound can rise
  L2, G  100,003 spans each, distinct traces, half of them ERROR, ring at w0
  T    25,013 spans over the ring at w0 and 25,013 over the ring at w0 + a
       (a = n_windows / 2, 1 for one window), sparse fresh traces, half ERROR:
       ends in retired, surviving and new windows
  U    20,011 spans, ring at w0 + a
  V    20,011 spans, ring at w0 + a + n_windows + 3

  advance(w0); F, L2; check A; G; advance(w0 + a); T; check B; forced reclaim
  and an advance by zero; U; check C; advance(w0 + a + n_windows + 3); V; check D

Nothing reads a window between G and the advance, so G's ERROR counts, ERROR
slab partials and raised bounds sit in the slots that retire.

References (reference(), computed once per row and shared by the modes): the
RED series come from an oracle fed every span, reset at each flush
(exponential rows: parity_util._check over the batches since the last flush);
the sketches from a second oracle fed, per batch, only the spans whose end lay
inside the ring as it stood when that batch went in -- the engine drops the
others as window_out_of_range, and a later advance must not resurrect them.
Every comparison is bit-exact but the float sums (parity_util.SUM_RTOL, with
check_against_oracle's rule for a wrapped u64 sum).

tests/test_ring_walk.py proves on the oracles alone that the batches can catch
what they are there for; tests/test_gpu_ring.py runs the walk on the GPU.
"""
import ctypes as C
import functools
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

import pyoracle
from geometry_util import RING_ROWS, check_expo, concat, config_of, expected_oor, make_batch, ring_start, unit_div
from parity_util import assert_red_equal
from spanagg import Group, SpanAggError, SpanBatch, _lib

# hll_filtered after G.  True: the kernel reads the lower bounds (the v2 small
# kernels, ExpoSmall's two included, and the binned / dense scatter).  False,
# decided from the code (P.hll_lb and P.hll_filt appear in ingest_v2_kernel and
# its epilogues and in sa_bt_scatter.h only):
#   ring_linear    small_fn returns ingest_lds_kernel without a bin table; it
#                  neither loads P.hll_lb nor counts into P.hll_filt
#   ring_expo_hbm  launch_expo sends an ExpoHbm engine's sketches through
#                  launch_ingest_hbm (ingest_hbm_kernel, RED part off): per-span
#                  atomic register raises, no bounds
#   ring_part      part_scatter_kernel raises registers per span, no bounds
#   ring_atomic    ingest_hbm_kernel
FILTERS = dict(ring_default=True, ring_512=True, ring_1024_noerr=True, ring1=True, ring_linear=False,
               ring_expo_spec=True, ring_expo_generic=True, ring_expo_hbm=False, ring_part=False, ring_atomic=False,
               ring_binned=True, ring_dense=True)
assert set(FILTERS) == set(RING_ROWS)

ORDER = ("F", "L2", "A", "G", "T", "B", "U", "C", "V", "D")  # batches and checks in walk order


def in_ring(batch, cfg, base) -> SpanBatch:
    """The spans whose end lies in the ring of n_windows windows from `base`."""
    w = batch.end_ns // np.uint64(cfg.window_ns)
    keep = (w >= base) & (w < base + cfg.n_windows)
    return SpanBatch(*[c[keep] for c in batch.columns()])


@functools.lru_cache(maxsize=2)
def walk(row):
    """The row's batches (seed: crc32 of the row name), the ring base each is
    ingested under and the base at each check."""
    r, cfg = RING_ROWS[row], config_of(row)
    rng = np.random.default_rng(zlib.crc32(row.encode()))
    w0, W, nk = ring_start(cfg), cfg.n_windows, r["n_keys"]
    regs = (W * cfg.n_services) << cfg.hll_p
    a = 1 if W == 1 else W // 2
    b = {}
    b["F"] = make_batch(rng, max(r["fill"] * regs, 200_000), cfg, nk, w0=w0, distinct_traces=True)
    for name in ("L2", "G"):
        b[name] = make_batch(rng, 100_003, cfg, nk, error_share=0.5, w0=w0, distinct_traces=True)
    b["T"] = concat([make_batch(rng, 25_013, cfg, nk, error_share=0.5, w0=w0),
                     make_batch(rng, 25_013, cfg, nk, error_share=0.5, w0=w0 + a)])
    b["U"] = make_batch(rng, 20_011, cfg, nk, w0=w0 + a)
    b["V"] = make_batch(rng, 20_011, cfg, nk, w0=w0 + a + W + 3)
    w1, w2 = w0 + a, w0 + a + W + 3
    base = dict(F=w0, L2=w0, A=w0, G=w0, T=w1, B=w1, U=w1, C=w1, V=w2, D=w2)
    return SimpleNamespace(row=row, cfg=cfg, w0=w0, W=W, a=a, regs=regs, batches=b, base=base)


def _series(o, cfg):
    """The oracle's RED series; a series whose u64 ns sum wrapped takes that
    sum as its float reference (geometry_util.check_against_oracle)."""
    ora = o.series()
    wrapped = ora["sum_go"] * unit_div(cfg) >= 0.999 * 2.0 ** 64
    ora["sum_go"] = np.where(wrapped, ora["sum_ns"] / unit_div(cfg), ora["sum_go"])
    return ora


def _windows(o, base, W):
    seen = set(o.window_ids())
    return {w: o.window(w) if w in seen else None for w in range(base, base + W)}


@functools.lru_cache(maxsize=2)
def reference(row):
    """What every check of the walk must see: per check the RED series since
    the previous flush (None on exponential rows), the batches behind them,
    the sketches of the ring's windows (None: never touched) and the stats.
    Also the sketch oracle's ring after F and the windows about to retire
    after G (tests/test_ring_walk.py)."""
    wk = walk(row)
    cfg = wk.cfg
    mk = lambda: pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    o_red, o_sk = mk(), mk()
    ref, since, oor = {}, [], 0
    for name in ORDER:
        base = wk.base[name]
        if name in wk.batches:
            b = wk.batches[name]
            o_red.ingest(b)
            o_sk.ingest(in_ring(b, cfg, base))
            oor += expected_oor([b], cfg, base)
            since.append(name)
            if name == "F":
                ref["after_F"] = _windows(o_sk, base, wk.W)
            if name == "G":
                ref["after_G"] = _windows(o_sk, base, wk.W)
            continue
        st = o_red.stats()
        ref[name] = SimpleNamespace(
            series=None if cfg.exp_max_size else _series(o_red, cfg), since=tuple(since),
            n=sum(len(wk.batches[s]) for s in since),
            zero=sum(int((wk.batches[s].key_hash == 0).sum()) for s in since),
            windows=_windows(o_sk, base, wk.W),
            stats=dict(spans=st["spans"], zero_key=st["zero_key"], invalid_service=st["invalid_service"],
                       window_out_of_range=oor, window_base=base, dropped_table_full=0))
        o_red.reset_red()
        since = []
    return ref


def slices(n, parts, rng):
    """Ragged slices at even offsets: device columns stay 16-byte aligned."""
    cuts = np.sort(rng.choice(np.arange(2, n, 2), size=parts - 1, replace=False))
    return [(int(a), int(b)) for a, b in zip(np.concatenate([[0], cuts]), np.concatenate([cuts, [n]]))]


class DeviceFeed:
    """The walk's batches on the GPU, copied once.  Consecutive launches
    alternate between two non-default streams that waited for the copies;
    nothing here synchronises with the host afterwards.  graph: every batch
    but F goes in as three ragged slices through ingest_device_many (F through
    ingest_device: L2 and G stay the second and third launch groups)."""

    def __init__(self, e, wk, graph=False):
        import torch
        dev = torch.device("cuda", 0)
        self.e, self.graph, self.cols, self.cuts, self.launches = e, graph, {}, {}, 0
        for name, b in wk.batches.items():
            key = b.key_hash
            if e.dense:  # indices for hashes, bound before the first launch
                key, new_i, new_h = e.ids.encode(key)
                if len(new_i):
                    e.bind_ids(new_i, new_h)
            self.cols[name] = [torch.from_numpy(np.ascontiguousarray(c).view(np.int64 if c.dtype == np.uint64
                                                                             else np.int32)).to(dev)
                               for c in (key,) + b.columns()[1:]]
            self.cuts[name] = slices(len(b), 3, np.random.default_rng(zlib.crc32((wk.row + name).encode())))
        self.streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        for s in self.streams:
            s.wait_stream(torch.cuda.current_stream(dev))  # (the columns' copies)

    def __call__(self, name):
        s = self.streams[self.launches % 2].cuda_stream
        self.launches += 1
        cols = self.cols[name]
        if self.graph and name != "F":
            self.e.ingest_device_many([tuple(c[a:b] for c in cols) for a, b in self.cuts[name]], stream=s)
        else:
            self.e.ingest_device(*cols, stream=s)


def _read_ring(e, base, W):
    return {w: e.window_read(w) for w in range(base, base + W)}


def _assert_ring(reads, windows, what):
    for w, sk in reads.items():
        if windows[w] is None:
            assert not sk.hll.any(), ("hll", what, w)
            assert not sk.cms.any(), ("cms", what, w)
        else:
            hll, cms = windows[w]
            assert np.array_equal(sk.hll, hll), ("hll", what, w)
            assert np.array_equal(sk.cms, cms), ("cms", what, w)


def _assert_stats(e, want, what):
    st = e.stats()
    assert {k: st[k] for k in want} == want, (what, st)
    return st


def _check(e, wk, ref, name):
    """Flushes and compares RED, every window of the ring and the stats with
    the reference of check `name`; returns the window reads."""
    s, cfg = ref[name], wk.cfg
    if cfg.exp_max_size:
        res = e.flush_exp()
        check_expo(res, concat([wk.batches[b] for b in s.since]), cfg.exp_max_size, cfg.unit == "s")
        assert int(res.count.sum()) == s.n - s.zero, name
    else:
        res = e.flush()
        assert_red_equal(res, s.series, unit_div=unit_div(cfg))
        assert int(res.calls.sum()) == s.n - s.zero, name
    reads = _read_ring(e, wk.base[name], wk.W)
    _assert_ring(reads, s.windows, name)
    _assert_stats(e, s.stats, name)
    return reads


def _raises(code, call):
    with pytest.raises(SpanAggError) as x:
        call()
    assert x.value.code == code, x.value


def _same(reads, again):
    for w, sk in reads.items():
        assert np.array_equal(sk.hll, again[w].hll) and np.array_equal(sk.cms, again[w].cms), w


def run_walk(e, row, feed, filter_after="G"):
    """Drives engine `e` (fresh, of row's config) through the walk; feed(name)
    ingests batch `name`.  filter_after: the batch after which hll_filtered
    must have moved on the kernels that filter.

    `e` may be a Group of such engines (tests/test_gpu_group_shards.py): the
    forced reclaim then goes to every member, and hll_filtered need not have
    moved -- a member sees 1/n of the fill batch, so "every register >= 1
    after F" does not hold for each member; it still must be 0 on the rows
    that do not filter."""
    wk, ref = walk(row), reference(row)
    group = isinstance(e, Group)
    cfg, w0, W, a = wk.cfg, wk.w0, wk.W, wk.a
    w2 = w0 + a + W + 3
    zeros = dict.fromkeys(range(w0, w2 + W))  # (any window of the walk: never touched)

    def filtered(after):
        n = e.stats()["hll_filtered"]
        if not FILTERS[row]:
            assert n == 0, (after, n)
        elif after == filter_after and not group:
            assert n > 0, after

    e.window_advance(w0)
    feed("F")
    feed("L2")
    _check(e, wk, ref, "A")  # (the reads fold every window's ERROR state)

    # the third launch: the first whose bounds are sure to cover F.  It leaves
    # ERROR counts, ERROR slab partials and bounds >= 1 in the slots about to
    # retire; nothing reads them, and on the device paths nothing waits for it
    feed("G")
    e.window_advance(w0 + a)
    for w in range(w0, w0 + a):
        _raises(_lib.SA_ERANGE, lambda: e.window_read(w))
    _assert_ring(_read_ring(e, w0 + W, a), zeros, "exposed")
    assert e.stats()["window_base"] == w0 + a
    filtered("G")  # (advance leaves the counter alone: this is G's)

    feed("T")
    reads_b = _check(e, wk, ref, "B")  # the flush: G + T
    filtered("T")

    # a forced reclaim folds every window's per-slot ERROR counts under the
    # key its slot holds now, then empties the key table
    if group:
        for i in range(e.size):  # (a group has no reclaim of its own)
            assert e.lib.sa_reclaim_keys(C.c_void_p(e.lib.sa_group_member(e._h, i)), 1) == 0, i
        assert e.stats()["n_keys"] == 0
    elif e.dense:
        _raises(_lib.SA_ESTATE, lambda: e.reclaim_keys(force=True))
    else:
        e.reclaim_keys(force=True)
        assert e.stats()["n_keys"] == 0
    e.window_advance(w0 + a)  # by zero
    again = _read_ring(e, w0 + a, W)
    _assert_ring(again, ref["B"].windows, "after reclaim")
    _same(reads_b, again)

    feed("U")  # keys re-insert, possibly elsewhere: folded ERROR counts neither move nor double
    _check(e, wk, ref, "C")

    e.window_advance(w2)  # past the whole ring
    _assert_ring(_read_ring(e, w2, W), zeros, "jump")
    feed("V")
    reads_d = _check(e, wk, ref, "D")
    filtered("V")

    if row == "ring_512":
        _raises(_lib.SA_EINVAL, lambda: e.window_advance(w2 - 1))
        _raises(_lib.SA_EINVAL, lambda: e.window_advance(2 ** 64 // cfg.window_ns + 1))
        again = _read_ring(e, w2, W)
        _assert_ring(again, ref["D"].windows, "after refused advances")
        _same(reads_d, again)
        _assert_stats(e, ref["D"].stats, "after refused advances")
