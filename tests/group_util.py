"""Engine groups: trace ids built to land on a chosen member, batches that
spread them badly, the members' own counters, and the fold of the members'
exponential histograms restated.

A group's merged results cannot show its shard rule: every merge is a sum or a
maximum, so a rule that is wrong but the same everywhere gives the same flush
and the same windows.  Only the members' counters can (member_stats), and only
on trace ids whose shard is known beforehand.

shard_words(n, targets, family, rng): trace_w1 values w with w % n ==
targets[i] (Python's int %; tests/test_group_host.py checks that on the
result).  Families, by the 32-bit halves csrc/sa_shard.h's shard_of works on:

  low       high word 0
  high      low word 0.  hi * 2^32 % n takes every value only when 2^32 % n is
            a unit mod n; for the other targets (all but 0 when n is a power of
            two) the low word is the target itself: the least that reaches it
  max_hi    high word 2^32 - 1
  max_lo    low word 2^32 - 1; a target the high word cannot reach takes the
            largest low word that does (within n of 2^32 - 1)
  near_top  within 2n of 2^64
  mixed     both words drawn

targets(n, count, dist): round_robin; skew0 (all on shard 0, the last span on
n - 1); two_only (shards 1 and n - 1 alternating, every other shard empty);
one_each (one span per shard first, the rest on n - 1).

SMALL is the configuration of the tests where only the sharding matters;
their workloads draw from at most 40 keys.

The fold (fold / fold_all, csrc/sa_shard.h's expo_fold in Python): both
histograms go to the smaller scale (indices shift down, floor), the index
ranges unite, and the least further downscale that fits max_size applies.
wrong= builds it with a known mistake (WRONG): "toward_zero" shifts negative
indices toward zero, "no_downscale" leaves the further downscale out,
"larger_scale" goes to the larger scale (the coarser histogram's indices stay
as they are).  fold_cases draws the case families of FAMILIES.
"""
import ctypes as C

import numpy as np

from geometry_util import key_pool, ring_start
from spanagg import SpanBatch, _lib, pack_meta

U64 = np.uint64
FAMILIES_W1 = ("low", "high", "max_hi", "max_lo", "near_top", "mixed")
DISTS = ("round_robin", "skew0", "two_only", "one_each")
TOP32 = (1 << 32) - 1

SMALL = dict(n_windows=2, hll_p=4, n_services=2, cms_d=1, cms_w=2, bounds=(1.0,), key_capacity=64)
N_KEYS = 40


# ---- trace ids by shard ----------------------------------------------------------------------------------------

def _lo_for(n, want, rng, top=False):
    """A low word with lo % n == want[i]: drawn, or (top) the largest one."""
    want = want.astype(U64)
    kmax = (U64(TOP32) - want) // U64(n)
    k = kmax if top else (rng.random(len(want)) * (kmax.astype(np.float64) + 1)).astype(U64)
    return want + U64(n) * np.minimum(k, kmax)


def _hi_for(n, want, rng):
    """A high word with hi * 2^32 % n == want[i] and which targets have one."""
    r32 = (1 << 32) % n
    first = np.full(n, -1, dtype=np.int64)
    for h in range(n - 1, -1, -1):
        first[(h * r32) % n] = h
    h0 = first[want]
    ok = h0 >= 0
    k = rng.integers(1, (TOP32 - n) // n, len(want))  # (hi >= n: never the zero word)
    return np.where(ok, h0 + n * k, 0).astype(U64), ok


def shard_words(n, targets, family, rng) -> np.ndarray:
    t = np.asarray(targets, dtype=np.int64)
    assert family in FAMILIES_W1 and ((t >= 0) & (t < n)).all()
    m, r32 = len(t), U64((1 << 32) % n)
    if family == "near_top":  # 2^64 - 1 - j, j < 2n
        top = ((1 << 64) - 1) % n
        j = (top - t) % n + n * rng.integers(0, 2, m)
        return U64((1 << 64) - 1) - j.astype(U64)
    if family in ("high", "max_lo"):
        lo_fixed = 0 if family == "high" else TOP32
        hi, ok = _hi_for(n, (t - lo_fixed) % n, rng)
        other = rng.integers(1, 1 << 32, m, dtype=U64)  # the high word where it cannot decide
        hi = np.where(ok, hi, other)
        rest = (t - ((hi % U64(n)) * r32 % U64(n)).astype(np.int64)) % n
        lo = np.where(ok, U64(lo_fixed), rest.astype(U64) if family == "high" else _lo_for(n, rest, rng, top=True))
        return (hi << U64(32)) | lo.astype(U64)
    hi = dict(low=np.zeros(m, dtype=U64), max_hi=np.full(m, TOP32, dtype=U64),
              mixed=rng.integers(0, 1 << 32, m, dtype=U64))[family]
    rest = (t - ((hi % U64(n)) * r32 % U64(n)).astype(np.int64)) % n
    return (hi << U64(32)) | _lo_for(n, rest, rng)


def mixed_words(n, targets, rng) -> np.ndarray:
    """shard_words with the families mixed: span i takes family i mod 6."""
    t = np.asarray(targets, dtype=np.int64)
    out = np.zeros(len(t), dtype=U64)
    for f, family in enumerate(FAMILIES_W1):
        out[f::len(FAMILIES_W1)] = shard_words(n, t[f::len(FAMILIES_W1)], family, rng)
    return out


def targets(n, count, dist) -> np.ndarray:
    assert dist in DISTS and count >= 1
    if dist == "round_robin":
        return np.arange(count) % n
    if dist == "skew0":
        t = np.zeros(count, dtype=np.int64)
        t[-1] = n - 1
        return t
    if dist == "two_only":
        return np.where(np.arange(count) % 2 == 0, 1 % n, n - 1)
    t = np.full(count, n - 1, dtype=np.int64)
    t[:min(n, count)] = np.arange(min(n, count))
    return t


def shard_counts(w1, n) -> list:
    """Spans per member: w % n in exact u64 arithmetic (tests/test_group_host.py
    holds it against Python's int % n)."""
    return np.bincount((np.asarray(w1, dtype=U64) % U64(n)).astype(np.int64), minlength=n).tolist()


def batch_for(cfg, w1, rng, keys=None, zero_share=0.01, max_log2=34, dur=None) -> SpanBatch:
    """One span per trace id of w1, shaped by cfg: keys uniform over `keys`
    (key_pool(40) by default; an array of len(w1): as given), ~1 % key 0,
    services uniform, ends uniform over the ring at ring_start, durations `dur`
    or log-uniform 1 ns .. 2^max_log2 ns with 5 % zero, a third of the spans
    ERROR."""
    n = len(w1)
    pool = key_pool(N_KEYS) if keys is None else np.asarray(keys, dtype=U64)
    key = pool.copy() if keys is not None and len(pool) == n else pool[rng.integers(0, len(pool), n)]
    key[rng.random(n) < zero_share] = 0
    end = U64(ring_start(cfg) * cfg.window_ns) + rng.integers(0, cfg.n_windows * cfg.window_ns, n, dtype=U64)
    if dur is None:
        dur = np.floor(2.0 ** rng.uniform(0, max_log2, n)).astype(U64)
        dur[rng.random(n) < 0.05] = 0
    meta = pack_meta(rng.integers(0, cfg.n_services, n), rng.integers(0, 6, n), rng.integers(0, 3, n))
    return SpanBatch(key, end - dur, end, rng.integers(0, 2**64, n, dtype=U64), np.asarray(w1, dtype=U64), meta)


def member_stats(g) -> list:
    """Every member's sa_get_stats, through sa_group_member."""
    out = []
    for i in range(g.size):
        h = g.lib.sa_group_member(g._h, i)
        assert h, i
        s = _lib.sa_stats()
        rc = g.lib.sa_get_stats(C.c_void_p(h), C.byref(s))
        assert rc == 0, (i, rc)
        out.append({name: int(getattr(s, name)) for name, _ in _lib.sa_stats._fields_ if name != "pad"})
    return out


def member_reclaim(g, force=True):
    """sa_reclaim_keys on every member (a group has no call of its own)."""
    for i in range(g.size):
        rc = g.lib.sa_reclaim_keys(C.c_void_p(g.lib.sa_group_member(g._h, i)), int(force))
        assert rc == 0, (i, rc)


# ---- the fold ----------------------------------------------------------------------------------------------------

WRONG = ("toward_zero", "no_downscale", "larger_scale")
FAMILIES = ("log_uniform", "pow2_pm1", "near_1ms", "half_zeros", "outlier", "zero_shard", "one_shard", "skew0")
MAX_SIZES = (2, 3, 4, 5, 7, 8, 12, 160, 161, 4096)


def _shr(v, k, wrong=None):
    if wrong == "toward_zero" and v < 0:
        return -((-v) >> k)
    return v >> k  # Python's >> floors


def fold(a, h, max_size, wrong=None):
    """Folds histogram h (a pyoracle.expo_series dict) into accumulator a (the
    same keys; None: empty) and returns the accumulator."""
    if h["count"] == 0:
        return a
    counts = [int(x) for x in h["counts"]]
    if a is None:
        return dict(count=h["count"], zero_count=h["zero_count"], scale=h["scale"] if counts else 20,
                    offset=h["offset"] if counts else 0, counts=counts)
    a = dict(a, count=a["count"] + h["count"], zero_count=a["zero_count"] + h["zero_count"])
    if not counts:
        return a
    if not a["counts"]:
        return dict(a, scale=h["scale"], offset=h["offset"], counts=counts)
    s = max(a["scale"], h["scale"]) if wrong == "larger_scale" else min(a["scale"], h["scale"])
    ka, kd = max(0, a["scale"] - s), max(0, h["scale"] - s)
    lo = min(_shr(a["offset"], ka, wrong), _shr(h["offset"], kd, wrong))
    hi = max(_shr(a["offset"] + len(a["counts"]) - 1, ka, wrong), _shr(h["offset"] + len(counts) - 1, kd, wrong))
    c = 0
    while hi - lo >= max_size and wrong != "no_downscale":
        lo, hi, c = _shr(lo, 1, wrong), _shr(hi, 1, wrong), c + 1
    if hi - lo >= max_size:  # (no_downscale only: wider than any histogram may be; not built)
        return dict(a, scale=s, offset=lo, counts=[-1])
    out = [0] * (hi - lo + 1)
    for i, v in enumerate(a["counts"]):
        out[_shr(a["offset"] + i, ka + c, wrong) - lo] += v
    for i, v in enumerate(counts):
        out[_shr(h["offset"] + i, kd + c, wrong) - lo] += v
    return dict(a, scale=s - c, offset=lo, counts=out)


def fold_all(members, max_size, wrong=None):
    a = None
    for h in members:
        a = fold(a, h, max_size, wrong)
    return a


def same_histogram(a, ora) -> bool:
    """count, zero count, scale, offset and buckets, bit for bit (a: fold's
    accumulator or None, ora: expo_series of the whole stream)."""
    if a is None:
        return ora["count"] == 0
    if (a["count"], a["zero_count"]) != (ora["count"], ora["zero_count"]):
        return False
    if not a["counts"] and not len(ora["counts"]):
        return True  # (only zeros: no bucket, the scale says nothing)
    return (a["scale"], a["offset"], a["counts"]) == (ora["scale"], ora["offset"], [int(x) for x in ora["counts"]])


def _cap_large(d, rng):
    """At most one duration of 2^58 ns or more and eight of 2^52 ns or more
    (expo_geometry_util's rule: the exact u64 ns sum is held against a float64
    sum); the others are drawn again below 2^52."""
    for floor_, limit in ((1 << 58, 1), (1 << 52, 8)):
        idx = np.flatnonzero(d >= U64(floor_))[limit:]
        d[idx] = np.floor(2.0 ** rng.uniform(0, 52, len(idx))).astype(U64)
    return d


def series_durations(family, rng, m) -> np.ndarray:
    """m durations (ns) of one series of a family."""
    logu = lambda k: np.maximum(np.floor(2.0 ** rng.uniform(0, 62, k)), 1).astype(U64)
    if family == "pow2_pm1":
        d = (U64(1) << rng.integers(1, 58, m).astype(U64)) + rng.integers(-1, 2, m).astype(np.int64).astype(U64)
    elif family == "near_1ms":
        d = (1_000_000 + rng.integers(-10, 11, m)).astype(U64)
    elif family == "half_zeros":
        d = logu(m)
        d[rng.random(m) < 0.5] = 0
    elif family == "outlier":
        d = np.full(m, int(logu(1)[0] >> U64(4)) + 1, dtype=U64)
        d[rng.integers(0, m)] = logu(1)[0]
    else:
        d = logu(m)
    return _cap_large(d, rng)


def series_shards(family, rng, m, n, d) -> np.ndarray:
    """The member each of the series' m spans goes to (and, for zero_shard,
    the durations of that member's spans set to zero, in place)."""
    sh = rng.integers(0, n, m)
    if family == "zero_shard":
        z = int(rng.integers(0, n))
        sh[0], sh[-1] = z, (z + 1) % n  # the zero member and another both hold spans
        d[sh == z] = 0
    elif family == "one_shard":
        sh[:] = rng.integers(0, n)
    elif family == "skew0":
        sh[:] = 0
        sh[-1] = n - 1
    return sh


def fold_cases(seed, count):
    """count cases, every family x max_size x unit in turn, 2..5 members, 2..40
    spans (near_1ms: 20): dicts of family, max_size, unit_s, n, dur, shard."""
    rng = np.random.default_rng(seed)
    for c in range(count):
        family = FAMILIES[c % len(FAMILIES)]
        M = MAX_SIZES[(c // len(FAMILIES)) % len(MAX_SIZES)]
        unit_s = bool((c // (len(FAMILIES) * len(MAX_SIZES))) % 2)
        n = int(rng.integers(2, 6))
        m = 20 if family == "near_1ms" else int(rng.integers(2, 41))
        d = series_durations(family, rng, m)
        sh = series_shards(family, rng, m, n, d)
        yield dict(family=family, max_size=M, unit_s=unit_s, n=n, dur=d, shard=sh)
