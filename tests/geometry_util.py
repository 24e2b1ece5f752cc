"""Non-default engine geometries: the matrix rows, a workload shaped by a row's
config, and the comparison with the CPU oracle.

ROWS is shared by tests/test_path_decision.py (the decisions on the CPU) and
tests/test_gpu_geometry.py (the kernels on the GPU); RING_ROWS, the small rings
of the moving-ring walk (tests/ring_util.py), by tests/test_path_decision.py,
tests/test_ring_walk.py and tests/test_gpu_ring.py (tests/hll_util.py adds six
rows of the same form for hll_p 4 and 18).  Each row's expectation is
written from the rules, not read from the code:

  cap   = next power of two >= 1.25 x key_capacity (>= 16; SA_OPT_DENSE_IDS: >= 2^19)
  X     = 24,704 (kLdsExtraBytes, tests/test_path_decision.py)
  lds   = cap*16 + cap*ceil(nbk/2)*4 + X        (Small, <= 147,456)
          cap*41 + X                            (ExpoSmall)
  small kernel  linear    some power-of-two bin of nanoseconds holds > 2 thresholds
                default   cap 2,048, ceil(nbk/2) = 9, p = 14
                512       2*lds <= 163,840, i.e. lds <= 81,920
                1024      the rest
  expo kernel   specialised for cap 2,048 and p = 14, generic otherwise
  HBM kernels   the 16-bound instance for 16 bounds, none negative; generic otherwise
  filter        regs = n_windows * n_services * 2^p; shift = the smallest s in
                10..p with regs >> s <= 2,048, n = regs >> shift; off when there is none
  ERROR table   small tables only: n_windows * cap < 65,535

The arithmetic of every row:

  default17   1,250 -> 2,048 slots; nbk 17; p 14: default.  regs 16*64*2^14 = 2^24 -> (13, 2048)
  half17      1,000 -> 1,024; 16,384 + 36,864 + X = 77,952: 512.  16*20*2^12 >> 10 = 1,280
  wide10      1,875 -> 2,048; nbk 10: 32,768 + 40,960 + X = 98,432: 1024.  p 8 < 10: off
              (-1.5 is the one negative bound; -0.0 is not below zero)
  cap4096     3,750 -> 4,096; nbk 4: 65,536 + 32,768 + X = 123,008: 1024.  16*2*2^18 = 2^23 -> (12, 2048)
              16*4,096 = 65,536 >= 65,535: no ERROR table
  cap4096w8   8*2*2^18 = 2^22 -> (11, 2048); 8*4,096 = 32,768: ERROR table
  nbk63       250 -> 256; nbk 63: 4,096 + 256*128 + X = 61,568: 512.  1.25*2^k and 1.75*2^k
              ns are the two thresholds of bin k: a bin table
  nbk63wide   500 -> 512: 8,192 + 65,536 + X = 98,432: 1024
  nbk1        1,250 -> 2,048; nbk 1: 32,768 + 8,192 + X = 65,664: 512
  linear      1.1e6 .. 1.4e6 ns all in [2^20, 2^21): four thresholds in a bin, linear
  linear_part 125,000 -> 2^17 and 375,000 -> 2^19, nbk 7, no bin table: Partitioned
  svc64k      default table, p 4: 2,048*52 + X = 131,200: 1024.  p 4 < 10: off
  ring1       as svc64k with p 10.  1*1*2^10 >> 10 = 1 -> (10, 1)
  part_generic  2^17, nbk 10 <= 17, below 2^19: Partitioned.  16*7*2^11 >> 10 = 224
  atomic_*    nbk 31 and 63 > 17: Atomic
  binned5     2^19, nbk 5, a bin table (1e6 .. 1e9 ns in four bins): Binned.  16*12*2^10 >> 10 = 192
  binned_neg  16*12*2^14 = 3,145,728: >> 10 = 3,072, >> 11 = 1,536 -> (11, 1536)
  dense5      binned5 with SA_OPT_DENSE_IDS
  expo_spec   2,048 slots, p 14: specialised
  expo_generic  500 -> 512: 512*41 + X = 45,696.  16*20*2^12 >> 10 = 1,280
  expo_p      2,048 slots, p 10: generic.  16*64*2^10 >> 10 = 1,024

RING_ROWS (n_windows stated in every row; rings small enough to raise every
register of):

  ring_default   1,250 -> 2,048 slots; nbk 17, p 14: default; 32,768 + 73,728 + X = 131,200.
                 regs 2*1*2^14 = 32,768 >> 10 = 32 -> (10, 32).  2*2,048 = 4,096: ERROR table
  ring_512       1,000 -> 1,024; 16,384 + 36,864 + X = 77,952 <= 81,920: 512.  4*2*2^11 = 16,384 >> 10 = 16
  ring_1024_noerr  1,875 -> 2,048; nbk 10: 32,768 + 40,960 + X = 98,432: 1024.  32*1*2^10 >> 10 = 32 (shift 10 = p).
                 32*2,048 = 65,536 >= 65,535: no ERROR table
  ring1          ROWS["ring1"]: one window, every advance clears the whole ring
  ring_linear    1,250 -> 2,048; nbk 7: 32,768 + 32,768 + X = 90,240; 1.1e6 .. 1.4e6 ns in one bin: linear.
                 4*2*2^11 >> 10 = 16.  4*2,048 = 8,192: ERROR table (allocated; the linear kernel counts per span)
  ring_expo_spec   2,048 slots, p 14: specialised; 2,048*41 + X.  2*1*2^14 >> 10 = 32
  ring_expo_generic  500 -> 512: 512*41 + X = 45,696; p 11: generic.  4*2*2^11 >> 10 = 16
  ring_expo_hbm  ring_expo_spec with SA_OPT_EXPO_HBM: ExpoHbm, its sketches through the HBM kernel.  The default 16
                 bounds, none negative: the HBM kernels' rule gives the 16-bound instance (bounds16).  Not an
                 LDS table: no ERROR table, no dynamic LDS.  Its 2,048-slot table takes the small rows' 700 keys
  ring_part      125,000 -> 2^17; nbk 10 <= 17, below 2^19: Partitioned; one negative bound: generic.  (10, 16)
  ring_atomic    2^17; nbk 31 > 17: Atomic; 30 bounds: generic.  (10, 16)
  ring_binned    375,000 -> 2^19; nbk 5, a bin table, 4 windows <= 1,024: Binned.  (10, 16)
  ring_dense     ring_binned with SA_OPT_DENSE_IDS
"""
import functools

import numpy as np

import pyoracle
from parity_util import _check as check_expo
from parity_util import assert_red_equal
from spanagg import Config, SpanBatch, bucket_thresholds, pack_meta
from spanagg._lib import OPT_DENSE_IDS, OPT_EXPO_HBM

DEFAULT = (2, 4, 6, 8, 10, 50, 100, 200, 400, 800, 1000, 1400, 2000, 5000, 10000, 15000)
NINE = (-1.5, -0.0, 0.1, 0.3, 1.0000001, 3.3, 7.77, 1e3, 2.5e6)
SIXTY_TWO = tuple(sorted(m * 2.0 ** k / 1e6 for k in range(10, 41) for m in (1.25, 1.75)))
THIRTY = tuple(2.0 ** i / 8 for i in range(30))
CROWDED6 = (1.1, 1.2, 1.3, 1.4, 50, 500)
OFF = (0, 0)  # no HLL filter

SMALL_THICK, HBM_THICK, THIN = 3_000_017, 1_000_003, 20_011


def _row(cfg, path, kernel, log2cap, lb, error_table=False, lds=0):
    small = path in ("Small", "ExpoSmall")
    kcap = cfg.get("key_capacity", 1000)
    cfg = dict({"n_windows": 16}, **cfg)
    return dict(cfg=cfg, path=path, kernel=kernel, log2cap=log2cap, lb=lb, error_table=error_table, lds=lds,
                n_keys=int(0.7 * kcap) if small else 60_000, thick=SMALL_THICK if small else HBM_THICK)


ROWS = {
    "default17": _row(dict(key_capacity=1000), "Small", "small_default", 11, (13, 2048), True, 131_200),
    "half17": _row(dict(key_capacity=800, hll_p=12, n_services=20), "Small", "small_512", 10, (10, 1280), True, 77_952),
    "wide10": _row(dict(key_capacity=1500, bounds=NINE, unit="s", hll_p=8, cms_d=1, cms_w=2, n_services=300),
                   "Small", "small_1024", 11, OFF, True, 98_432),
    "cap4096": _row(dict(key_capacity=3000, bounds=(1, 10, 100), hll_p=18, n_services=2),
                    "Small", "small_1024", 12, (12, 2048), False, 123_008),
    "cap4096w8": _row(dict(key_capacity=3000, bounds=(1, 10, 100), hll_p=18, n_services=2, n_windows=8),
                      "Small", "small_1024", 12, (11, 2048), True, 123_008),
    "nbk63": _row(dict(key_capacity=200, bounds=SIXTY_TWO, cms_d=8, cms_w=64), "Small", "small_512", 8, (13, 2048),
                  True, 61_568),
    "nbk63wide": _row(dict(key_capacity=400, bounds=SIXTY_TWO, cms_d=8, cms_w=64), "Small", "small_1024", 9,
                      (13, 2048), True, 98_432),
    "nbk1": _row(dict(key_capacity=1000, bounds=()), "Small", "small_512", 11, (13, 2048), True, 65_664),
    "linear": _row(dict(key_capacity=1000, bounds=CROWDED6), "Small", "small_linear", 11, (13, 2048), True, 90_240),
    "linear_part17": _row(dict(key_capacity=100_000, bounds=CROWDED6), "Partitioned", "bounds_generic", 17, (13, 2048)),
    "linear_part19": _row(dict(key_capacity=300_000, bounds=CROWDED6), "Partitioned", "bounds_generic", 19, (13, 2048)),
    "svc64k": _row(dict(key_capacity=1000, hll_p=4, n_services=65536), "Small", "small_1024", 11, OFF, True, 131_200),
    "ring1": _row(dict(key_capacity=1000, n_windows=1, window_ns=7_000_000_007, hll_p=10, n_services=1),
                  "Small", "small_1024", 11, (10, 1), True, 131_200),
    "part_generic": _row(dict(key_capacity=100_000, bounds=NINE, unit="s", hll_p=11, n_services=7),
                         "Partitioned", "bounds_generic", 17, (10, 224)),
    "atomic_nbk31": _row(dict(key_capacity=100_000, bounds=THIRTY), "Atomic", "bounds_generic", 17, (13, 2048)),
    "atomic_nbk63": _row(dict(key_capacity=100_000, bounds=SIXTY_TWO), "Atomic", "bounds_generic", 17, (13, 2048)),
    "binned5": _row(dict(key_capacity=300_000, bounds=(1, 10, 100, 1000), hll_p=10, cms_d=2, cms_w=64, n_services=12),
                    "Binned", "bounds_generic", 19, (10, 192)),
    "binned_neg": _row(dict(key_capacity=300_000, bounds=NINE, unit="s", n_services=12),
                       "Binned", "bounds_generic", 19, (11, 1536)),
    "dense5": _row(dict(key_capacity=300_000, bounds=(1, 10, 100, 1000), hll_p=10, cms_d=2, cms_w=64, n_services=12,
                        options=OPT_DENSE_IDS), "Dense", "bounds_generic", 19, (10, 192)),
    "expo_spec": _row(dict(key_capacity=1000, exp_max_size=160), "ExpoSmall", "expo_specialised", 11, (13, 2048),
                      True, 2048 * 41 + 24_704),
    "expo_generic": _row(dict(key_capacity=400, exp_max_size=20, hll_p=12, n_services=20),
                         "ExpoSmall", "expo_generic", 9, (10, 1280), True, 45_696),
    "expo_p": _row(dict(key_capacity=1500, exp_max_size=160, hll_p=10, unit="s"),
                   "ExpoSmall", "expo_generic", 11, (10, 1024), True, 2048 * 41 + 24_704),
}


def _ring(cfg, *expect, fill=24, n_keys=None):
    """A RING_ROWS row: n_windows stated; `fill` = the fill batch's spans per
    register of the ring (ring_util.walk)."""
    assert "n_windows" in cfg
    r = dict(_row(cfg, *expect), fill=fill)
    if n_keys is not None:
        r["n_keys"] = n_keys
    return r


_RING_EXPO = dict(key_capacity=1000, exp_max_size=160, hll_p=14, n_services=1, n_windows=2)
_RING_BINNED = dict(key_capacity=300_000, bounds=(1, 10, 100, 1000), hll_p=11, n_services=2, n_windows=4)

RING_ROWS = {
    "ring_default": _ring(dict(key_capacity=1000, hll_p=14, n_services=1, n_windows=2),
                          "Small", "small_default", 11, (10, 32), True, 131_200),
    "ring_512": _ring(dict(key_capacity=800, hll_p=11, n_services=2, n_windows=4),
                      "Small", "small_512", 10, (10, 16), True, 77_952),
    "ring_1024_noerr": _ring(dict(key_capacity=1500, bounds=NINE, unit="s", hll_p=10, n_services=1, n_windows=32),
                             "Small", "small_1024", 11, (10, 32), False, 98_432),
    "ring1": dict(ROWS["ring1"], fill=24),
    "ring_linear": _ring(dict(key_capacity=1000, bounds=CROWDED6, hll_p=11, n_services=2, n_windows=4),
                         "Small", "small_linear", 11, (10, 16), True, 90_240),
    "ring_expo_spec": _ring(_RING_EXPO, "ExpoSmall", "expo_specialised", 11, (10, 32), True, 2048 * 41 + 24_704),
    "ring_expo_generic": _ring(dict(key_capacity=400, exp_max_size=20, hll_p=11, n_services=2, n_windows=4),
                               "ExpoSmall", "expo_generic", 9, (10, 16), True, 45_696),
    "ring_expo_hbm": _ring(dict(_RING_EXPO, options=OPT_EXPO_HBM), "ExpoHbm", "bounds16", 11, (10, 32), n_keys=700),
    "ring_part": _ring(dict(key_capacity=100_000, bounds=NINE, unit="s", hll_p=11, n_services=2, n_windows=4),
                       "Partitioned", "bounds_generic", 17, (10, 16)),
    "ring_atomic": _ring(dict(key_capacity=100_000, bounds=THIRTY, hll_p=11, n_services=2, n_windows=4),
                         "Atomic", "bounds_generic", 17, (10, 16)),
    "ring_binned": _ring(_RING_BINNED, "Binned", "bounds_generic", 19, (10, 16)),
    "ring_dense": _ring(dict(_RING_BINNED, options=OPT_DENSE_IDS), "Dense", "bounds_generic", 19, (10, 16)),
}


def config_of(row) -> Config:
    return Config(**(RING_ROWS.get(row) or ROWS[row])["cfg"])


def assert_geometry(e, row, rows=None):
    """Engine.debug_geometry() against the row's expectation (ROWS or RING_ROWS,
    or another matrix `rows` of the same form)."""
    r, g = (rows or {}).get(row) or RING_ROWS.get(row) or ROWS[row], e.debug_geometry()
    assert (g["path"], g["kernel"], g["log2cap"]) == (r["path"], r["kernel"], r["log2cap"]), g
    assert (g["lb_shift"], g["lb_n"]) == r["lb"], g
    assert g["error_table"] == r["error_table"], g
    if r["lds"]:
        assert g["lds_bytes"] == r["lds"], g
    # 256-thread workgroups on the atomic path (an ExpoHbm engine's sketches run its kernel), 1,024
    # everywhere else but the half-block kernel
    hbm = r["path"] in ("Atomic", "ExpoHbm")
    assert g["block"] == (512 if r["kernel"] == "small_512" else 256 if hbm else 1024), g
    # small tables: one resident round of workgroups, at most two per CU
    assert 0 < g["grid_max"] and (g["grid_max"] <= 512 or r["path"] not in ("Small", "ExpoSmall")), g
    return g


def ring_start(cfg) -> int:
    """The ring's first window: late enough for an end time to have a start
    2^62 ns before it."""
    return (1 << 62) // cfg.window_ns + 2


def unit_div(cfg) -> float:
    return 1e9 if cfg.unit == "s" else 1e6


@functools.lru_cache(maxsize=None)
def key_pool(n_keys) -> np.ndarray:
    """n_keys distinct non-zero series ids -- the same for every batch of a
    row, so a row's batches together stay within its key_capacity."""
    pool = np.random.default_rng([n_keys, 0x5EED]).integers(1, 2**64, 2 * n_keys + 16, dtype=np.uint64)
    pool = pool[np.sort(np.unique(pool, return_index=True)[1])][:n_keys]  # distinct, in drawn order
    assert len(pool) == n_keys
    return pool


def _pick(rng, values, n):
    return np.asarray(values, dtype=np.uint64)[rng.integers(0, len(values), n)]


def make_batch(rng, n, cfg, n_keys, error_share=0.3, w0=None, distinct_traces=False) -> SpanBatch:
    """n spans shaped by cfg.  Keys: n_keys distinct non-zero ids (key_pool), half the
    spans on 8 hot ones, ~1 % key 0.  Services uniform, ~1 % one past the last.
    Ends uniform over the ring from window w0 (ring_start by default), ~1 % in
    the window before or after it, the first four on the first and last
    nanosecond of the first and last window.  Durations: ~10 % on t - 1, t,
    t + 1 of the finite bucket thresholds t, 2 % zero, 2 % with end < start,
    1 % of 2^62 ns, the rest log-uniform from 1 ns to 4 x the largest threshold
    (10 s without bounds).  Traces from a pool of n / 8 ids (distinct_traces:
    one per span).  ERROR with probability error_share.

    Of the 1 % of 2^62 ns, one span per series stays (the others keep their
    log-uniform duration): the engine sums exact u64 ns, which four such spans
    in a series wrap, and the sums are compared with Go's float64 sums."""
    w0 = ring_start(cfg) if w0 is None else w0
    W, wns, S = cfg.n_windows, cfg.window_ns, cfg.n_services
    pool = key_pool(n_keys)
    hot = rng.random(n) < 0.5
    key = np.where(hot, pool[rng.integers(0, min(8, n_keys), n)], pool[rng.integers(0, n_keys, n)])
    key[rng.random(n) < 0.01] = 0

    svc = rng.integers(0, S, n).astype(np.uint32)
    if S < 65536:
        svc[rng.random(n) < 0.01] = S

    end = np.uint64(w0 * wns) + rng.integers(0, W * wns, n, dtype=np.uint64)
    out = rng.random(n) < 0.01
    side = np.where(rng.random(n) < 0.5, w0 - 1, w0 + W).astype(np.uint64)
    end = np.where(out, side * np.uint64(wns) + rng.integers(0, wns, n, dtype=np.uint64), end)
    edges = np.array([w0 * wns, (w0 + 1) * wns - 1, (w0 + W - 1) * wns, (w0 + W) * wns - 1], dtype=np.uint64)
    m = min(4, n)
    end[:m], svc[:m] = edges[:m], 0

    thr, _ = bucket_thresholds(cfg.bounds, cfg.unit)
    finite = [int(t) for t in thr if int(t) < (1 << 61)]
    top = 4 * max(finite) if finite and max(finite) > 0 else 10_000_000_000
    dur = np.exp(rng.uniform(0.0, np.log(float(top)), n)).astype(np.uint64)
    dur = np.clip(dur, 1, top)
    u = rng.random(n)
    near = sorted({d for t in finite for d in (t - 1, t, t + 1) if d >= 0})
    if near:
        sel = u < 0.10
        dur[sel] = _pick(rng, near, int(sel.sum()))
    dur[(u >= 0.10) & (u < 0.12)] = 0
    huge = np.flatnonzero((u >= 0.14) & (u < 0.15))
    huge = huge[np.unique(key[huge], return_index=True)[1]]  # one per series
    dur[huge] = 1 << 62
    start = end - dur
    back = (u >= 0.12) & (u < 0.14)  # end < start: the duration is 0
    start[back] = end[back] + rng.integers(1, 1_000_000, int(back.sum()), dtype=np.uint64)

    if distinct_traces:
        t0, t1 = rng.integers(0, 2**64, n, dtype=np.uint64), rng.integers(0, 2**64, n, dtype=np.uint64)
    else:
        np_ = max(1, n // 8)
        p0, p1 = rng.integers(0, 2**64, np_, dtype=np.uint64), rng.integers(0, 2**64, np_, dtype=np.uint64)
        ti = rng.integers(0, np_, n)
        t0, t1 = p0[ti], p1[ti]
    status = np.where(rng.random(n) < error_share, 2, rng.integers(0, 2, n)).astype(np.uint32)
    status[:m] = 2  # the ring's edge spans show in the count-min cells too
    return SpanBatch(key, start, end, t0, t1, pack_meta(svc, rng.integers(0, 6, n), status))


def concat(batches) -> SpanBatch:
    return SpanBatch(*[np.concatenate(c) for c in zip(*[b.columns() for b in batches])])


def expected_oor(batches, cfg, w0) -> int:
    """Spans of a valid service whose end lies outside the ring (as
    test_gpu_parity.expected_oor counts them)."""
    n = 0
    for b in batches:
        w = b.end_ns // np.uint64(cfg.window_ns)
        ok = (b.meta & np.uint32(0xFFFF)) < cfg.n_services
        n += int((ok & ~((w >= w0) & (w < w0 + cfg.n_windows))).sum())
    return n


def check_against_oracle(engine, batches, cfg, w0, earlier=()):
    """Flushes the engine and compares everything with the oracle: the RED
    series (or exponential histograms) of `batches` -- what was ingested since
    the last flush; the HLL registers and count-min cells of every ring window
    and the stats over `earlier` + `batches`.  Returns the flush result."""
    batches, everything = list(batches), list(earlier) + list(batches)
    o = pyoracle.Oracle(cfg.bounds, cfg.unit, cfg.hll_p, cfg.cms_d, cfg.cms_w, cfg.window_ns, cfg.n_services)
    for b in earlier:
        o.ingest(b)
    o.reset_red()
    for b in batches:
        o.ingest(b)
    n = sum(len(b) for b in batches)
    st_o = o.stats()
    zero_now = sum(int((b.key_hash == 0).sum()) for b in batches)
    if cfg.exp_max_size:
        res = engine.flush_exp()
        check_expo(res, concat(batches), cfg.exp_max_size, cfg.unit == "s")
        assert int(res.count.sum()) == n - zero_now
    else:
        res = engine.flush()
        ora = o.series()
        # The ABI's sum is sum_ns / divisor, sum_ns an exact u64 (include/spanagg.h).
        # A series whose durations pass 2^64 ns within one interval (a hot
        # key's log-uniform tail under a bound of weeks) wraps it, in the
        # oracle's sum_ns as in the engine's -- the two are compared exactly.
        # For such a series the float reference is the oracle's own u64 sum
        # over the divisor, not Go's unbounded float64 sum.
        wrapped = ora["sum_go"] * unit_div(cfg) >= 0.999 * 2.0 ** 64
        ora["sum_go"] = np.where(wrapped, ora["sum_ns"] / unit_div(cfg), ora["sum_go"])
        assert_red_equal(res, ora, unit_div=unit_div(cfg))
        assert int(res.calls.sum()) == n - zero_now
    seen = set(o.window_ids())
    for wid in range(w0, w0 + cfg.n_windows):
        sk = engine.window_read(wid)
        if wid in seen:
            hll, cms = o.window(wid)
            assert np.array_equal(sk.hll, hll), ("hll", wid)
            assert np.array_equal(sk.cms, cms), ("cms", wid)
        else:
            assert not sk.hll.any() and not sk.cms.any(), wid
    st = engine.stats()
    assert st["spans"] == st_o["spans"] == sum(len(b) for b in everything)
    assert st["zero_key"] == st_o["zero_key"]
    assert st["invalid_service"] == st_o["invalid_service"]
    assert st["window_out_of_range"] == expected_oor(everything, cfg, w0)
    assert st["dropped_table_full"] == 0
    return res
