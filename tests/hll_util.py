"""Trace ids crafted for the HyperLogLog side: every rho on every ingest path.

A random trace id reaches rho = r with probability 2^-r, so random workloads
never run the kernels' rho code past the high twenties, and the HLL lower
bounds they produce sit at 0 to 3.  The builders here run xxh64 of the 16
trace-id bytes backwards (trace_with_hash) and so put a span on any (register
index, rho) they like.  tests/test_hll_ids_host.py proves on the CPU that the
batches are what they claim (by the plain-Python forward reference below and
by the oracle); tests/test_gpu_hll_ids.py runs them through the kernels.

The forward reference is written from xxHash's published description of
XXH64 for an input of 16 bytes and seed 0 (two 8-byte lanes folded into
PRIME64_5 + 16, then the avalanche), and from the HyperLogLog rule the
engine documents: with x the hash and p = hll_p,

  index = x >> (64 - p)
  rho   = clz(((x << p) | 1 << (p - 1)) mod 2^64) + 1        1 .. 65 - p

Registers are named (window, service, index); their position in the engine's
register array is ((window & (n_windows - 1)) * n_services + service) << p |
index -- slot order, which is also the order of the lower bounds' sub-blocks
(sub-block j: positions [j << lb_shift, (j + 1) << lb_shift)).

Every family returns (SpanBatch, claims); claims is an int64 array [n, 4] of
the (window, service, index, rho) of each span, in the batch's order.  All
spans have a valid service, an end inside the ring of n_windows windows from
`w0` and a non-zero key of geometry_util.key_pool(n_keys).

HLL_ROWS: six more ring rows for the ends of hll_p (4 and 18) on the v2
kernel's lean and plain forms and on the binned scatter.  Worked out from the
rules at the top of geometry_util.py (n_windows = 2, the default bounds: nbk 17):

  p4_lean     1,000 -> 1,024 slots; 16,384 + 1,024*9*4 + X = 77,952 <= 81,920: 512.  p 4 < 10: no filter.
              2*1,024 = 2,048: ERROR table.  regs 2*8*16 = 256
  p18_lean    as p4_lean; regs 2*1*2^18 = 2^19 >> 10 = 512 <= 2,048 -> (10, 512)
  p4_plain    1,250 -> 2,048; 32,768 + 73,728 + X = 131,200 > 81,920, p is not 14: 1024.  off.  4,096: ERROR table
  p18_plain   as p4_plain; (10, 512)
  p4_binned   375,000 -> 2^19; nbk 5, a bin table, 2 windows: Binned.  off
  p18_binned  (10, 512)

At p = 4 a window has 16 registers a service: 2 windows x 8 services x 16 =
256 registers, of which every_rho takes 3 x 61 + 3, half_boundary 20 and
shared_word 6 -- each on a register of its own.
"""
import zlib
from types import SimpleNamespace

import numpy as np

from geometry_util import _RING_BINNED, OFF, RING_ROWS, ROWS, THIN, _ring, concat, key_pool, make_batch
from spanagg import Config, SpanBatch, pack_meta

HLL_ROWS = {
    "p4_lean": _ring(dict(key_capacity=800, hll_p=4, n_services=8, n_windows=2),
                     "Small", "small_512", 10, OFF, True, 77_952),
    "p18_lean": _ring(dict(key_capacity=800, hll_p=18, n_services=1, n_windows=2),
                      "Small", "small_512", 10, (10, 512), True, 77_952),
    "p4_plain": _ring(dict(key_capacity=1000, hll_p=4, n_services=8, n_windows=2),
                      "Small", "small_1024", 11, OFF, True, 131_200),
    "p18_plain": _ring(dict(key_capacity=1000, hll_p=18, n_services=1, n_windows=2),
                       "Small", "small_1024", 11, (10, 512), True, 131_200),
    "p4_binned": _ring(dict(_RING_BINNED, n_windows=2, hll_p=4, n_services=8), "Binned", "bounds_generic", 19, OFF),
    "p18_binned": _ring(dict(_RING_BINNED, n_windows=2, hll_p=18, n_services=1),
                        "Binned", "bounds_generic", 19, (10, 512)),
}
ALL_ROWS = {**RING_ROWS, **HLL_ROWS}
# The kernels that read the lower bounds (ring_util.FILTERS says why the other four do not): of those, the
# rows whose geometry has a filter at all
FILTER_ROWS = tuple(r for r, v in ALL_ROWS.items() if v["lb"] != OFF
                    and r not in ("ring_linear", "ring_expo_hbm", "ring_part", "ring_atomic"))
FLOOR = 20  # filter_floor's F
# The rows above all have sub-blocks of 2^10 registers: 64 quads, one per lane.  The two-phase bound
# (sa_device.h hll_lb_pre / hll_lb_finish) takes four quads a lane up front and reads the rest in a second loop,
# which only sub-blocks of more than 256 quads reach: geometry_util.ROWS["default17"], 16 windows x 64 services x
# 2^14 registers = 2^24 -> (13, 2048), sub-blocks of 8,192 registers = 512 quads.  Its ring is floored in part.
DEEP = "default17"


def filters(row) -> bool:
    """Whether the row's kernel skips HLL updates on the strength of the lower bounds."""
    return row in FILTER_ROWS or row == DEEP


def row_of(row):
    return ALL_ROWS[row] if row in ALL_ROWS else {DEEP: ROWS[DEEP]}[row]


def config_of(row) -> Config:
    return Config(**row_of(row)["cfg"])


# ---------------------------------------------------------------- the hash, forwards and backwards

_M64 = (1 << 64) - 1
_P1, _P2, _P3, _P4, _P5 = (0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0x85EBCA77C2B2AE63,
                           0x27D4EB2F165667C5)  # xxh64's primes


def _rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & _M64


def _inv(a):
    return pow(a, -1, 1 << 64)


def xxh64_16(w0, w1):
    """XXH64, seed 0, of the 16 bytes w0, w1 (little-endian u64 words), on Python integers."""
    h = (_P5 + 16) & _M64
    for w in (w0, w1):
        h ^= _rotl(w * _P2 & _M64, 31) * _P1 & _M64
        h = (_rotl(h, 27) * _P1 + _P4) & _M64
    h ^= h >> 33
    h = h * _P2 & _M64
    h ^= h >> 29
    h = h * _P3 & _M64
    return h ^ (h >> 32)


def index_rho(x, p):
    """(register index, rho) of hash x at precision p."""
    y = ((x << p) | (1 << (p - 1))) & _M64
    return x >> (64 - p), 64 - y.bit_length() + 1


def trace_with_hash(x, w0):
    """trace_w1 such that xxh64 of the 16 trace-id bytes (w0, w1 little-endian,
    seed 0) is x: the avalanche and the second lane's round undone."""
    h = x
    h ^= h >> 32
    h = h * _inv(_P3) & _M64
    h ^= h >> 29
    h ^= h >> 58
    h = h * _inv(_P2) & _M64
    h ^= h >> 33
    h1 = (_rotl(((_P5 + 16) & _M64) ^ (_rotl(w0 * _P2 & _M64, 31) * _P1 & _M64), 27) * _P1 + _P4) & _M64
    r = _rotl((h - _P4) * _inv(_P1) & _M64, 64 - 27) ^ h1
    return _rotl(r * _inv(_P1) & _M64, 64 - 31) * _inv(_P2) & _M64


def _u(v):
    return np.uint64(v)


def _rotl_np(v, r):
    return (v << _u(r)) | (v >> _u(64 - r))


def _lane1_np(w0):
    """The hash state after the first 8-byte lane."""
    return _rotl_np(_u((_P5 + 16) & _M64) ^ (_rotl_np(w0 * _u(_P2), 31) * _u(_P1)), 27) * _u(_P1) + _u(_P4)


def xxh64_16_np(w0, w1):
    """xxh64_16 on uint64 arrays."""
    w0, w1 = np.asarray(w0, np.uint64), np.asarray(w1, np.uint64)
    with np.errstate(over="ignore"):
        h = _lane1_np(w0)
        h = _rotl_np(h ^ (_rotl_np(w1 * _u(_P2), 31) * _u(_P1)), 27) * _u(_P1) + _u(_P4)
        h ^= h >> _u(33)
        h = h * _u(_P2)
        h ^= h >> _u(29)
        h = h * _u(_P3)
        return h ^ (h >> _u(32))


def trace_with_hash_np(x, w0):
    """trace_with_hash on uint64 arrays."""
    x, w0 = np.asarray(x, np.uint64), np.asarray(w0, np.uint64)
    with np.errstate(over="ignore"):
        h = x ^ (x >> _u(32))
        h = h * _u(_inv(_P3))
        h ^= h >> _u(29)
        h ^= h >> _u(58)
        h = h * _u(_inv(_P2))
        h ^= h >> _u(33)
        r = _rotl_np((h - _u(_P4)) * _u(_inv(_P1)), 64 - 27) ^ _lane1_np(w0)
        return _rotl_np(r * _u(_inv(_P1)), 64 - 31) * _u(_inv(_P2))


def index_rho_np(x, p):
    """index_rho on a uint64 array: (index, rho) as int64 arrays."""
    x = np.asarray(x, np.uint64)
    y = (x << _u(p)) | _u(1 << (p - 1))  # never 0: a binary search for the leading one
    clz = np.zeros(len(x), np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        z = (y >> _u(64 - s)) == 0
        clz += np.where(z, s, 0)
        y = np.where(z, y << _u(s), y)
    return (x >> _u(64 - p)).astype(np.int64), clz + 1


# ---------------------------------------------------------------- rings, registers, spans

class Ring:
    """The registers of cfg's ring from window w0, by position in the engine's array."""

    def __init__(self, cfg, w0):
        self.cfg, self.w0, self.W, self.S, self.p = cfg, int(w0), cfg.n_windows, cfg.n_services, cfg.hll_p
        self.m = 1 << self.p
        self.regs = self.W * self.S * self.m
        self.top = 65 - self.p  # the largest rho

    def pos(self, window, svc, index):
        return (((np.asarray(window, np.int64) & (self.W - 1)) * self.S + np.asarray(svc, np.int64)) << self.p) | index

    def unpos(self, pos):
        """(window, service, index) of array positions."""
        pos = np.asarray(pos, np.int64)
        row = pos >> self.p
        window = self.w0 + ((row // self.S - self.w0) & (self.W - 1))
        return window, row % self.S, pos & (self.m - 1)

    @property
    def zero(self):
        """Position 0: slot 0, service 0, index 0 -- the byte idle lanes read."""
        return 0

    @property
    def last(self):
        """The last window's last service's last index."""
        return int(self.pos(self.w0 + self.W - 1, self.S - 1, self.m - 1))

    def take(self, used, n):
        """n positions not in `used` (a set, updated), spread evenly over the ring."""
        free = np.setdiff1d(np.arange(self.regs), np.fromiter(used, np.int64, len(used)))
        assert len(free) >= n, (len(free), n)
        got = free[(np.arange(n) * len(free)) // n]
        used.update(int(q) for q in got)
        return got


def hashes(p, index, rho, low):
    """Hashes with the given register index and rho whose bits below the
    leading one are those of `low` (for rho = 65 - p there is no leading one:
    the low 64 - p bits are zero and the sentinel ends the count)."""
    t = 64 - p
    index, rho, low = (np.asarray(a).astype(np.uint64) for a in (index, rho, low))
    assert ((rho >= 1) & (rho <= t + 1)).all() and (index < (1 << p)).all()
    lead = np.where(rho <= _u(t), _u(1) << (_u(t) - np.minimum(rho, _u(t))), _u(0))
    below = np.where(lead > 0, lead - _u(1), _u(0))
    return (index << _u(t)) | lead | (low & below)


ALT = 0x5555555555555555


def make_spans(cfg, n_keys, window, svc, x, salt=0):
    """One span per hash x: trace ids that hash to x, ends inside `window`,
    keys of the row's pool, a third of the spans ERROR."""
    n = len(x)
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        t0 = (i + _u(1 + salt)) * _u(0x9E3779B97F4A7C15) + _u(salt)
    t1 = trace_with_hash_np(x, t0)
    wns = _u(cfg.window_ns)
    end = np.asarray(window).astype(np.uint64) * wns + (i * _u(999_983) + _u(4321)) % wns
    dur = _u(1000) + (i % _u(53)) * _u(997_003)
    pool = key_pool(n_keys)
    key = pool[(np.arange(n) + salt) % min(n_keys, 64)]
    k = np.arange(n)
    meta = pack_meta(np.asarray(svc).astype(np.uint32), k % 6, np.where(k % 3 == 0, 2, k % 2))
    return SpanBatch(key, end - dur, end, t0, t1, meta)


def _family(ring, n_keys, pos, rho, low, salt):
    window, svc, index = ring.unpos(pos)
    x = hashes(ring.p, index, rho, low)
    batch = make_spans(ring.cfg, n_keys, window, svc, x, salt)
    return batch, np.stack([window, svc, index, np.asarray(rho, np.int64)], axis=1)


def claims_of(batch, cfg):
    """(window, service, index, rho) of every span of a batch, by the NumPy forward hash."""
    index, rho = index_rho_np(xxh64_16_np(batch.trace_w0, batch.trace_w1), cfg.hll_p)
    window = (batch.end_ns // _u(cfg.window_ns)).astype(np.int64)
    return np.stack([window, (batch.meta & np.uint32(0xFFFF)).astype(np.int64), index, rho], axis=1)


def expected_registers(ring, claims):
    """{window: [n_services][2^p] u8}: the maximum claimed rho per register."""
    out = {w: np.zeros((ring.S, ring.m), np.uint8) for w in range(ring.w0, ring.w0 + ring.W)}
    for w in out:
        c = claims[claims[:, 0] == w]
        np.maximum.at(out[w], (c[:, 1], c[:, 2]), c[:, 3].astype(np.uint8))
    return out


# ---------------------------------------------------------------- the families

def every_rho(cfg, w0, n_keys, touch_zero=True, used=None):
    """Every rho 1 .. 65 - p in three variants -- the bits below the leading
    one clear, set, alternating -- each (rho, variant) on a register of its
    own, spread evenly over the ring's windows and services.  The very last
    register (last window, last service, index 2^p - 1) takes rho 64 - p: the
    index bits, zeros and bit 0 of the hash, which alone decides.  The last
    position of the array, where that is another register, takes the largest
    rho; position 0 takes the largest rho when touch_zero, else no span at
    all."""
    ring = Ring(cfg, w0)
    used = set() if used is None else used
    end = ring.regs - 1
    used.update({ring.zero, ring.last, end})
    top = ring.top
    rho = np.repeat(np.arange(1, top + 1), 3)
    low = np.tile(np.array([0, _M64, ALT], np.uint64), top)
    pos = ring.take(used, len(rho))
    extra = [(ring.last, top - 1, 0)] + ([(end, top, 0)] if end != ring.last else [])
    if touch_zero:
        extra.append((ring.zero, top, 0))
    pos = np.concatenate([pos, np.array([e[0] for e in extra], np.int64)])
    rho = np.concatenate([rho, np.array([e[1] for e in extra], np.int64)])
    low = np.concatenate([low, np.array([e[2] for e in extra], np.uint64)])
    return _family(ring, n_keys, pos, rho, low, salt=1)


def half_boundary(cfg, w0, n_keys, used=None):
    """rho 31 .. 34: the leading one of x << p at bits 33, 32 (the high half is
    2 or 3, then 1) and 31, 30 (the high half is zero, the low half decides).
    Per rho five hashes that differ only below the leading one: nothing, every
    bit, alternating, only the low p bits of the hash (they end just above the
    sentinel and must not matter), and every bit but those.  The register
    indices alternate between all ones and zero: the index must not reach the
    high half."""
    ring = Ring(cfg, w0)
    used = set() if used is None else used
    pmask = (1 << ring.p) - 1
    lows = np.array([0, _M64, ALT, pmask, _M64 ^ pmask], np.uint64)
    rho = np.repeat(np.arange(31, 35), len(lows))
    low = np.tile(lows, 4)
    pos = ring.take(used, len(rho))
    # same windows and services, the index forced to all ones or zero where that register is still free
    want = (pos & ~np.int64(ring.m - 1)) | np.where(np.arange(len(pos)) % 2 == 0, ring.m - 1, 0)
    for k, q in enumerate(want):
        if int(q) not in used:
            used.discard(int(pos[k]))
            used.add(int(q))
            pos[k] = q
    return _family(ring, n_keys, pos, rho, low, salt=2)


def _ladder(top, n=64):
    """n rhos ascending from 1 to the largest."""
    return np.round(np.linspace(1, top, n)).astype(np.int64)


def shared_word(cfg, w0, n_keys, used=None):
    """Three blocks of consecutive spans (keep each whole and in order):
      word     the four registers of one aligned 32-bit word, 64 spans each,
               rhos ascending, descending and (twice) shuffled, interleaved
               register by register: 256 spans whose lanes raise one word at once
      same     one (register, rho) on all 128 spans of a wave step
      ceiling  a register taken to 65 - p, then every lower rho sent at it
    Returns ([word, same, ceiling] batches, their claims)."""
    ring = Ring(cfg, w0)
    used = set() if used is None else used
    rng = np.random.default_rng(zlib.crc32(b"shared_word"))
    used.update({ring.zero, ring.last, ring.regs - 1})  # every_rho's
    taken = np.zeros(ring.regs, bool)
    taken[np.fromiter(used, np.int64, len(used))] = True
    free4 = np.flatnonzero(~taken.reshape(-1, 4).any(axis=1)) * 4  # the words nothing else uses
    word = int(free4[len(free4) // 2])
    used.update(range(word, word + 4))
    lad = _ladder(ring.top)
    rhos = np.stack([lad, lad[::-1], rng.permutation(lad), rng.permutation(lad)], axis=1).ravel()
    pos = np.tile(np.arange(word, word + 4), 64)
    out = [_family(ring, n_keys, pos, rhos, rng.integers(0, 2**64, len(pos), dtype=np.uint64), salt=3)]
    same, ceil = ring.take(used, 2)
    out.append(_family(ring, n_keys, np.full(128, same), np.full(128, 7),
                       rng.integers(0, 2**64, 128, dtype=np.uint64), salt=4))
    down = np.concatenate([[ring.top], np.arange(ring.top - 1, 0, -1), [ring.top - 1, 1]])
    out.append(_family(ring, n_keys, np.full(len(down), ceil), down,
                       rng.integers(0, 2**64, len(down), dtype=np.uint64), salt=5))
    return [b for b, _ in out], [c for _, c in out]


def crafted(cfg, w0, n_keys, touch_zero=True):
    """every_rho, half_boundary and shared_word on registers of their own:
    (singles, blocks, claims) -- singles one batch whose spans may go in any
    order, blocks the batches to keep whole, claims those of concat([singles] +
    blocks)."""
    used = set()
    blocks, cs = shared_word(cfg, w0, n_keys, used)  # first: an aligned word still free of the others
    b1, c1 = every_rho(cfg, w0, n_keys, touch_zero, used)
    b2, c2 = half_boundary(cfg, w0, n_keys, used)
    return concat([b1, b2]), blocks, np.concatenate([c1, c2] + cs)


def off_register(batch, cfg, pos, ring):
    """The batch without the spans that land on array position `pos` (or one of several)."""
    c = claims_of(batch, cfg)
    inside = (c[:, 1] < ring.S) & (c[:, 0] >= ring.w0) & (c[:, 0] < ring.w0 + ring.W)
    hit = inside & np.isin(ring.pos(c[:, 0], np.minimum(c[:, 1], ring.S - 1), c[:, 2]), pos)
    return SpanBatch(*[col[~hit] for col in batch.columns()])


def mixed(cfg, w0, n_keys, touch_zero=True, seed=0):
    """The crafted spans shuffled into a THIN random batch: a crafted span at
    position 0 and one at the last position, shared_word's blocks whole at
    multiples of 128.  Without touch_zero no span at all lands on position 0.
    Returns (the batch, the crafted spans alone as one batch, their claims)."""
    ring = Ring(cfg, w0)
    singles, blocks, claims = crafted(cfg, w0, n_keys, touch_zero)
    rng = np.random.default_rng([zlib.crc32(b"mixed"), seed])
    rand = make_batch(rng, THIN, cfg, n_keys, w0=w0)
    if not touch_zero:
        rand = off_register(rand, cfg, ring.zero, ring)
    if (len(rand) + len(singles) + sum(len(b) for b in blocks)) % 4 == 0:
        rand = rand.slice(0, len(rand) - 1)  # a ragged last tile
    pool = concat([rand, singles])
    perm = rng.permutation(len(pool))
    first, last = np.flatnonzero(perm >= len(rand))[[0, -1]]  # crafted spans: to the two ends
    perm[[0, first]] = perm[[first, 0]]
    perm[[-1, last]] = perm[[last, -1]]
    pool = SpanBatch(*[c[perm] for c in pool.columns()])
    cuts = [128 * k for k in (3, 41, 97)]
    parts, at = [], 0
    for cut, blk in zip(cuts, blocks):
        parts += [pool.slice(at, cut), blk]
        at = cut
    parts.append(pool.slice(at, len(pool)))
    batch = concat(parts)
    assert len(batch) % 4 != 0
    return batch, concat([singles] + blocks), claims


def invalid_spans(cfg, w0, n_keys, n=3001):
    """n spans none of which may reach a sketch: half with service n_services,
    half with an end one window before or after the ring; each carries a trace
    id of register index 0 and rho 64 - p or 65 - p."""
    ring = Ring(cfg, w0)
    k = np.arange(n)
    x = hashes(ring.p, np.zeros(n, np.int64), np.where(k % 4 < 2, ring.top, ring.top - 1), np.zeros(n, np.uint64))
    bad_svc = k % 2 == 0
    window = np.where(bad_svc, w0 + k % ring.W, np.where(k % 4 == 1, w0 - 1, w0 + ring.W))
    svc = np.where(bad_svc, ring.S, k % ring.S)
    return make_spans(cfg, n_keys, window, svc, x, salt=6)


# ---------------------------------------------------------------- the lower-bound filter

LOW_OFFSETS = (0, 15, 16 * 63, 16 * 64, 16 * 255 + 15, 16 * 256)


def filter_geometry(row):
    """(lb_shift, lb_n) of a row; for a row without a filter one sub-block of
    at most 1,024 registers, so the same batches can be built."""
    r, cfg = row_of(row), config_of(row)
    if r["lb"] != OFF:
        return r["lb"]
    regs = (cfg.n_windows * cfg.n_services) << cfg.hll_p
    shift = min(10, regs.bit_length() - 1)
    return shift, regs >> shift


def filter_floor(cfg, w0, n_keys, geometry, seed=0, partial=False):
    """The three batches that load and probe the lower-bound filter, for a
    filter of geometry = (lb_shift, lb_n):

      floor   one span per register of the ring: F = 20 everywhere but in the
              `low` registers, which take 1.  The low registers lie in
              sub-blocks spread over the ring, one each (several when there
              are fewer sub-blocks than offsets), at the offsets LOW_OFFSETS
              and 2^lb_shift - 1 that exist: the first and last byte of a
              16-byte quad, the last quad a lane reads in one pass, the first
              quad of the second loop, the sub-block's last byte
      probe   into every sub-block rho F - 1, F and F + 1 on three registers
              (not low ones), and rho 2 into every low register
      topup   a THIN random batch, less the spans that land on a low register

    partial: only the sub-blocks with a low register and two more are floored
    and probed, the rest of the ring stays 0 (a ring too large to fill: DEEP).

    Returns a namespace: floor, probe, topup (batches), floor_claims,
    probe_claims, low (array positions), up (the F + 1 registers' positions),
    floored (the sub-blocks the floor fills)."""
    ring = Ring(cfg, w0)
    shift, n_sb = geometry
    size = 1 << shift
    assert n_sb << shift == ring.regs
    rng = np.random.default_rng([zlib.crc32(b"filter_floor"), seed])
    offs = sorted({o for o in LOW_OFFSETS + (size - 1,) if o < size})
    low_sb = [(k * n_sb) // len(offs) for k in range(len(offs))]
    low = np.array([(sb << shift) + o for sb, o in zip(low_sb, offs)], np.int64)
    assert len(set(low)) == len(low)
    if n_sb > len(offs):
        assert len(set(low_sb)) == len(offs) and len(set(range(n_sb)) - set(low_sb)) > 0
    floored = np.arange(n_sb)
    if partial:
        more = [sb for sb in (low_sb[0] + 1, n_sb - 2) if sb not in low_sb]
        assert len(more) == 2
        floored = np.array(sorted(set(low_sb) | set(more)))
    order = rng.permutation(((floored[:, None] << shift) + np.arange(size)[None, :]).ravel())
    rho = np.where(np.isin(order, low), 1, FLOOR)
    floor, floor_claims = _family(ring, n_keys, order, rho, rng.integers(0, 2**64, len(order), dtype=np.uint64), salt=7)
    # three registers per sub-block, away from the low ones
    cand = np.array([o for o in (1 + (np.arange(12) * 83) % (size - 2)) if o not in offs][:3], np.int64)
    assert len(set(cand)) == 3
    base = (floored.astype(np.int64) << shift)[:, None]
    pos = np.concatenate([(base + cand[None, :]).ravel(), low])
    prho = np.concatenate([np.tile([FLOOR - 1, FLOOR, FLOOR + 1], len(floored)), np.full(len(low), 2)])
    up = (base[:, 0] + cand[2]).copy()
    mix = rng.permutation(len(pos))
    probe, probe_claims = _family(ring, n_keys, pos[mix], prho[mix], rng.integers(0, 2**64, len(pos), dtype=np.uint64),
                                  salt=8)
    topup = off_register(make_batch(rng, THIN, cfg, n_keys, w0=w0), cfg, low, ring)
    return SimpleNamespace(floor=floor, probe=probe, topup=topup, floor_claims=floor_claims, probe_claims=probe_claims,
                           low=low, up=up, ring=ring, floored=floored)


def topup_launches(lb_n, block):
    """Launches after which every sub-block has been refreshed since the floor
    landed: a launch refreshes grid x (block / 64) sub-blocks and the next one
    goes on where it stopped."""
    waves = block // 64
    return 1 + -(-lb_n // waves)


def equal_slices(batch, parts):
    n = len(batch)
    cuts = [(n * k) // parts for k in range(parts + 1)]
    return [batch.slice(a, b) for a, b in zip(cuts, cuts[1:])]


class CannotRaise:
    """Counts, launch by launch, the spans whose rho does not exceed their
    register's value at the start of their launch: what the filter may skip at
    the most.  The registers it keeps are the oracle's (the host test compares
    them)."""

    def __init__(self, cfg, w0):
        self.ring, self.count = Ring(cfg, w0), 0
        self.state = np.zeros(self.ring.regs, np.uint8)

    def launch(self, batch):
        ring = self.ring
        c = claims_of(batch, ring.cfg)
        ok = (c[:, 1] < ring.S) & (c[:, 0] >= ring.w0) & (c[:, 0] < ring.w0 + ring.W)
        c = c[ok]
        pos = ring.pos(c[:, 0], c[:, 1], c[:, 2])
        self.count += int((c[:, 3] <= self.state[pos]).sum())
        np.maximum.at(self.state, pos, c[:, 3].astype(np.uint8))
        return self.count

    def registers(self):
        """{window: [n_services][2^p]} of the ring."""
        ring = self.ring
        by_slot = self.state.reshape(ring.W, ring.S, ring.m)
        return {w: by_slot[w & (ring.W - 1)] for w in range(ring.w0, ring.w0 + ring.W)}


def after_advance_spans(cfg, w0, n_keys, geometry, blocks=3):
    """rho 1 and rho 2, one span per register of the first, a middle and the
    last sub-block (those that exist) of the ring at w0."""
    ring = Ring(cfg, w0)
    shift, n_sb = geometry
    sbs = sorted({0, n_sb // 2, n_sb - 1})[:blocks]
    pos = np.concatenate([np.arange(sb << shift, (sb + 1) << shift) for sb in sbs])
    rho = 1 + (pos % 3 == 0)
    return _family(ring, n_keys, pos, rho, np.full(len(pos), _M64, np.uint64), salt=9)
