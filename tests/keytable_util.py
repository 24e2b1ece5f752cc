"""Key tables on adversarial series ids: a NumPy mirror of the probe sequences
(csrc/sa_probe.h), key families built by inverting or searching the probe
hash, the rows whose kernels look keys up, and their workloads.

Shared by tests/test_keytable_host.py (the mirror against the compiled
functions, the families' properties, the rows' decisions and the oracle's
series counts, on the CPU) and tests/test_gpu_keytable.py (the kernels).

The probe hash of the small and HBM tables mixes x = lo ^ hi of a key's two
halves: h1 = x * 0x9E3779B1 (mod 2^32, odd multiplier: invertible), h2 from
h1's low 24 bits, b1 and b2 their top log2cap - 2 bits.  Keys with one x share
their whole sequence; an x whose h1 has chosen top bits is INV * h1.  The
binned table does the same inside a bin with y = (u32)m ^ (u32)(m >> 29).

KT_ROWS, each expectation written from the rules of tests/geometry_util.py
(X = 24,704; sketches kept small: 4 windows, p <= 11 and <= 2 services unless
the kernel's geometry needs p = 14):

  kt_min      8 -> 16 slots (4 buckets: every walk wraps); nbk 17: 256 + 576 + X = 25,536 <= 81,920: 512.
              regs 4*2*2^11 = 16,384 >> 10 = 16.  4*16 < 65,535: ERROR table
  kt_default  1,250 -> 2,048; nbk 17, p 14: default; 131,200.  4*1*2^14 >> 10 = 64.  4*2,048 = 8,192: ERROR table
  kt_512      geometry_util's half17 with small sketches: 1,000 -> 1,024; 77,952: 512.  (10, 16)
  kt_1024     wide10 with small sketches: 1,875 -> 2,048; nbk 10: 98,432 > 81,920: 1024.  4*1*2^10 >> 10 = 4
  kt_linear   1,250 -> 2,048; nbk 7: 90,240; CROWDED6 has four thresholds in one bin: linear.  (10, 16)
  kt_expo     expo_spec with small sketches: 2,048 slots, p 14: specialised; 2,048*41 + X.  (10, 64)
  kt_expo_generic  500 -> 512: 512*41 + X = 45,696; p 11: generic.  (10, 16)
  kt_part     1,639 + 410 = 2,049 -> 4,096 slots (the smallest HBM table): 4,096*52 + X > 147,456, nbk 17, below
              2^19: Partitioned; the default 16 bounds: bounds16.  (10, 16)
  kt_atomic   2,048 slots, nbk 31 > 17: 32,768 + 131,072 + X > 147,456: Atomic; 30 bounds: generic.  (10, 16)
  kt_expo_hbm kt_expo with SA_OPT_EXPO_HBM: ExpoHbm, its sketches through the HBM kernel (bounds16)
  kt_part17   125,000 -> 2^17; Partitioned, bounds16.  (10, 16)
  kt_binned   375,000 -> 2^19, SA_OPT_IDENTITY_IDS (m = key): Binned, 2,048 bins of 2^8 = 256 slots.  (10, 16)

Workgroups of one launch of n spans (csrc/engine_ingest.cpp plan_launch, the
partitioned and binned scatters): min(grid_max, ceil(n / tile)), tile = block x
spans per lane (2: the v2 and exponential small-table kernels; 4: the linear
kernel and the 256-thread HBM kernel), 1,024 spans per partitioned scatter
workgroup, 4,096 per binned one.
"""
import functools

import numpy as np

from geometry_util import CROWDED6, NINE, THIRTY, _row, key_pool, make_batch
from spanagg._lib import OPT_EXPO_HBM, OPT_IDENTITY_IDS

U32, U64 = np.uint32, np.uint64
MASK32 = 0xFFFFFFFF
M1, M2, M2B = 0x9E3779B1, 0x85EBCA, 0x85EBCA6B
INV_M1 = pow(M1, -1, 1 << 32)  # x = INV_M1 * h1 (mod 2^32)
PART_BIN_BITS = 11

# ---------------------------------------------------------------------------
# the mirror (u32 wrap arithmetic on u64 arrays, masked)


def _u64(a):
    return np.atleast_1d(np.asarray(a, dtype=U64))


def _mul32(a, c):
    return (a * U64(c)) & U64(MASK32)  # a < 2^32, c < 2^32: the product fits a u64


def probe_seq(key, log2cap):
    """(b1, b2, nbmask) of sa::probe_seq."""
    key = _u64(key)
    h1 = _mul32((key & U64(MASK32)) ^ (key >> U64(32)), M1)
    h2 = _mul32((h1 ^ (h1 >> U64(16))) & U64(0xFFFFFF), M2)
    sh = U64(34 - log2cap)
    return (h1 >> sh).astype(U32), (h2 >> sh).astype(U32), U32((1 << (log2cap - 2)) - 1)


def seq_slot(seq, i):
    """sa::seq_slot (and sa::bt_pos: the same walk) at position(s) i."""
    b1, b2, nbmask = seq
    i = np.asarray(i, dtype=np.int64)
    q = np.maximum(i - 4, 0)
    first = b1.astype(np.int64) * 4 + i
    rest = ((b2.astype(np.int64) + (q >> 2)) & int(nbmask)) * 4 + (q & 3)
    return np.where(i < 4, first, rest).astype(U32)


def max_probe_of(log2):
    return (1 << log2) + 4


def bt_seq(m, log2sb):
    """(b1, b2, nbmask) of sa::bt_seq."""
    m = _u64(m)
    h1 = _mul32((m & U64(MASK32)) ^ ((m >> U64(29)) & U64(MASK32)), M1)
    h2 = _mul32(h1 ^ (h1 >> U64(16)), M2B)
    sh = U64(34 - log2sb)
    return (h1 >> sh).astype(U32), (h2 >> sh).astype(U32), U32((1 << (log2sb - 2)) - 1)


bt_pos = seq_slot


def part_bin(key):
    return (_u64(key) >> U64(64 - PART_BIN_BITS)).astype(U32)


def bt_slot(m, log2sb, i):
    return (part_bin(m).astype(np.int64) << log2sb | bt_pos(bt_seq(m, log2sb), i).astype(np.int64)).astype(U32)


# ---------------------------------------------------------------------------
# key families


def _his(n, seed):
    """n distinct high halves: 0, 2^32 - 1, 1, 2^31 and random ones."""
    rng = np.random.default_rng([seed, 0xC4A1])
    hi = np.concatenate([np.array([0, MASK32, 1, 1 << 31], dtype=U64), rng.integers(0, 1 << 32, 2 * n + 8, dtype=U64)])
    hi = hi[np.sort(np.unique(hi, return_index=True)[1])][:n]
    assert len(hi) == n
    return hi


def keys_of_x(x, n, seed=0):
    """n distinct non-zero keys hi << 32 | (hi ^ x): all share lo ^ hi = x."""
    hi = _his(n + 1, seed)
    key = hi << U64(32) | (hi ^ U64(x))
    return key[key != 0][:n]


def _search_h1(log2cap, want, seed, fixed_b1=None):
    """The first h1 (from a seeded start; its top bits fixed_b1 if given) whose
    (b1, b2) satisfies want(b1, b2) -- found by evaluating the mix, not by
    reading a table."""
    sh = 34 - log2cap
    span = 1 << (sh if fixed_b1 is not None else 32)
    start = int(np.random.default_rng([seed, log2cap, 0x5EA]).integers(0, span))
    off, step = 0, 1 << 10
    while off < span:
        low = (np.arange(off, min(off + step, span), dtype=U64) + U64(start)) % U64(span)
        off, step = off + step, min(4 * step, 1 << 20)
        h1 = low if fixed_b1 is None else low | U64(fixed_b1 << sh)
        h2 = _mul32((h1 ^ (h1 >> U64(16))) & U64(0xFFFFFF), M2)
        ok = np.flatnonzero(want((h1 >> U64(sh)).astype(np.int64), (h2 >> U64(sh)).astype(np.int64)))
        if len(ok):
            return int(h1[ok[0]])
    raise LookupError(f"no such h1 at log2cap {log2cap}")


def x_of_h1(h1):
    return (h1 * INV_M1) & MASK32


def one_sequence(log2cap, n, seed=0):
    """n keys with one probe sequence, b1 != b2."""
    h1 = _search_h1(log2cap, lambda b1, b2: b1 != b2, seed)
    return keys_of_x(x_of_h1(h1), n, seed)


WRAP_VARIANTS = ("last", "b1_eq_b2", "b1_zero")


def wrapping(log2cap, n, variant="last", seed=0):
    """one_sequence with b2 the table's last bucket, so the walk wraps to
    bucket 0 right after it.  `last`: b1 any other bucket but 0; `b1_eq_b2`:
    b1 the last bucket too (positions 4-7 repeat 0-3); `b1_zero`: b1 = 0."""
    last = (1 << (log2cap - 2)) - 1
    if variant == "last":
        h1 = _search_h1(log2cap, lambda b1, b2: (b2 == last) & (b1 != last) & (b1 != 0), seed)
    else:
        h1 = _search_h1(log2cap, lambda b1, b2: b2 == last, seed, fixed_b1=last if variant == "b1_eq_b2" else 0)
    return keys_of_x(x_of_h1(h1), n, seed)


EDGES = np.array([1, 2**32 - 1, 2**32, 2**63, 2**64 - 2, 2**64 - 1], dtype=U64)


def halves(log2cap, limit=None):
    """Keys a compare of half a key would merge: two groups of four equal in
    their low 32 bits and distinct above, and two equal above and distinct
    below -- each group in one first-choice bucket, so the lookups meet (the
    partner's x is INV_M1 * h1' for an h1' with the same top bits); the edge
    values; and 8 base keys with their 64 single-bit neighbours."""
    rng = np.random.default_rng([log2cap, 0xA1F])
    sh = 34 - log2cap
    groups = []
    for g in range(4):
        lo, hi = (int(v) for v in rng.integers(1, 1 << 32, 2))
        top = ((((lo ^ hi) * M1) & MASK32) >> sh) << sh
        xs = [x_of_h1(top | int(v)) for v in rng.choice(1 << min(sh, 30), 3, replace=False)]
        if g < 2:  # same low half
            groups += [hi << 32 | lo] + [(lo ^ x) << 32 | lo for x in xs]
        else:      # same high half
            groups += [hi << 32 | lo] + [hi << 32 | (hi ^ x) for x in xs]
    bases = rng.integers(1, 2**64, 8, dtype=U64)
    near = (bases[:, None] ^ (U64(1) << np.arange(64, dtype=U64))[None, :]).reshape(-1)
    keys = np.concatenate([np.array(groups, dtype=U64), EDGES, bases, near])
    keys = keys[np.sort(np.unique(keys, return_index=True)[1])]
    keys = keys[keys != 0]
    return keys if limit is None else keys[:limit]


def one_bin_sequence(log2sb, n, wrap=True, seed=0):
    """n keys (m = key under SA_OPT_IDENTITY_IDS) with the same top bin bits and
    one bt_seq: y = (u32)m ^ (u32)(m >> 29) held equal while bits 32..52 vary.
    wrap: b2 the bin's last bucket, b1 another one."""
    sh, last = 34 - log2sb, (1 << (log2sb - 2)) - 1
    start = int(np.random.default_rng([seed, log2sb, 0xB17]).integers(0, 1 << 32))
    h1 = (np.arange(1 << 20, dtype=U64) + U64(start)) & U64(MASK32)
    h2 = _mul32(h1 ^ (h1 >> U64(16)), M2B)
    b1, b2 = h1 >> U64(sh), h2 >> U64(sh)
    ok = np.flatnonzero((b2 == last) & (b1 != last) if wrap else (b2 != last) & (b1 != b2))
    y = x_of_h1(int(h1[ok[0]]))
    top = 0x2A7  # the bin: bits 53..63
    mid = np.random.default_rng([seed, 0xB18]).choice(1 << 21, n, replace=False).astype(U64)  # bits 32..52
    # (u32)(m >> 29): bits 0-2 = m's bits 29-31, bits 3-23 = mid, bits 24-31 = the bin's low 8 bits
    above = (mid << U64(3)) | U64((top & 0xFF) << 24)
    lo = U64(y) ^ above          # right but for bits 0-2, which need lo's own bits 29-31
    lo = lo ^ (lo >> U64(29))    # bits 29-31 of lo are final: above has its bits 29-31 from the bin
    m = U64(top) << U64(53) | mid << U64(32) | lo
    assert len(np.unique(m)) == n and (m != 0).all()
    return m


# ---------------------------------------------------------------------------
# rows

_SMALL = dict(hll_p=11, n_services=2, n_windows=4)
_KT_EXPO = dict(key_capacity=1000, exp_max_size=160, hll_p=14, n_services=1, n_windows=4)

KT_ROWS = {
    "kt_min": _row(dict(_SMALL, key_capacity=8), "Small", "small_512", 4, (10, 16), True, 25_536),
    "kt_default": _row(dict(key_capacity=1000, hll_p=14, n_services=1, n_windows=4),
                       "Small", "small_default", 11, (10, 64), True, 131_200),
    "kt_512": _row(dict(_SMALL, key_capacity=800), "Small", "small_512", 10, (10, 16), True, 77_952),
    "kt_1024": _row(dict(key_capacity=1500, bounds=NINE, unit="s", hll_p=10, n_services=1, n_windows=4),
                    "Small", "small_1024", 11, (10, 4), True, 98_432),
    "kt_linear": _row(dict(_SMALL, key_capacity=1000, bounds=CROWDED6), "Small", "small_linear", 11, (10, 16), True,
                      90_240),
    "kt_expo": _row(_KT_EXPO, "ExpoSmall", "expo_specialised", 11, (10, 64), True, 2048 * 41 + 24_704),
    "kt_expo_generic": _row(dict(_SMALL, key_capacity=400, exp_max_size=20), "ExpoSmall", "expo_generic", 9, (10, 16),
                            True, 45_696),
    "kt_part": _row(dict(_SMALL, key_capacity=1639), "Partitioned", "bounds16", 12, (10, 16)),
    "kt_atomic": _row(dict(_SMALL, key_capacity=1000, bounds=THIRTY), "Atomic", "bounds_generic", 11, (10, 16)),
    "kt_expo_hbm": _row(dict(_KT_EXPO, options=OPT_EXPO_HBM), "ExpoHbm", "bounds16", 11, (10, 64)),
    "kt_part17": _row(dict(_SMALL, key_capacity=100_000), "Partitioned", "bounds16", 17, (10, 16)),
    "kt_binned": _row(dict(_SMALL, key_capacity=300_000, options=OPT_IDENTITY_IDS), "Binned", "bounds16", 19,
                      (10, 16)),
}
BINNED_LOG2SB = 19 - PART_BIN_BITS  # bins of 256 slots
TABLE_ROWS = [r for r in KT_ROWS if r != "kt_binned"]  # every row with the two-choice table over all its slots
FULL_ROWS = ["kt_min", "kt_default", "kt_1024", "kt_linear", "kt_expo", "kt_part", "kt_atomic", "kt_expo_hbm"]
THIN = 20_011


def cap_of(row):
    return 1 << KT_ROWS[row]["log2cap"]


def assert_kt_geometry(e, row):
    """geometry_util.assert_geometry for a KT_ROWS row."""
    r, g = KT_ROWS[row], e.debug_geometry()
    assert (g["path"], g["kernel"], g["log2cap"]) == (r["path"], r["kernel"], r["log2cap"]), g
    assert (g["lb_shift"], g["lb_n"]) == r["lb"], g
    assert g["error_table"] == r["error_table"], g
    if r["lds"]:
        assert g["lds_bytes"] == r["lds"], g
    hbm = r["path"] in ("Atomic", "ExpoHbm")
    assert g["block"] == (512 if r["kernel"] == "small_512" else 256 if hbm else 1024), g
    assert 0 < g["grid_max"] and (g["grid_max"] <= 512 or r["path"] not in ("Small", "ExpoSmall")), g
    return g


def workgroups(row, geometry, n):
    """The workgroups that share the key table in one launch of n spans."""
    r = KT_ROWS[row]
    if r["path"] == "Partitioned":
        per = 1024
    elif r["path"] == "Binned":
        per = 4096
    else:
        per = geometry["block"] * (4 if r["kernel"] == "small_linear" or r["path"] in ("Atomic", "ExpoHbm") else 2)
    return min(geometry["grid_max"], -(-n // per))


# ---------------------------------------------------------------------------
# workloads


def workload(rng, n, cfg, keys, w0=None, per_key=2):
    """n spans over exactly `keys`: geometry_util.make_batch's mix (its
    durations on the bucket edges, ends over the ring, ~1 % key 0, half the
    spans on the first 8 keys) with 10 % ERROR, its pool ids replaced one for
    one by `keys`, and per_key ordinary spans moved onto every key so none
    has fewer."""
    keys = np.asarray(keys, dtype=U64)
    K = len(keys)
    assert n >= (per_key + 1) * K + 64, (n, K)
    b = make_batch(rng, n, cfg, K, error_share=0.1, w0=w0)
    pool = key_pool(K)
    order = np.argsort(pool)
    idx = order[np.minimum(np.searchsorted(pool[order], b.key_hash), K - 1)]
    key = np.where(b.key_hash == 0, U64(0), keys[idx])
    ordinary = np.flatnonzero((key != 0) & (b.end_ns - b.start_ns != U64(1 << 62)))
    ordinary = ordinary[ordinary >= 4]  # (the ring's edge spans stay on their key)
    hot = np.isin(key[ordinary], keys[:8])  # the hot head gives its spans last
    take = np.concatenate([rng.permutation(ordinary[~hot]), rng.permutation(ordinary[hot])])[: per_key * K]
    assert len(take) == per_key * K
    key[take] = np.tile(keys, per_key)
    b.key_hash = np.ascontiguousarray(key)
    return b


def spans_for(n_keys):
    return max(THIN, 3 * n_keys + 1_031)


def hot_first(chain, filler):
    """chain + filler with four of each among the first 8 (the hot head)."""
    chain, filler = np.asarray(chain, dtype=U64), np.asarray(filler, dtype=U64)
    keys = np.concatenate([chain[:4], filler[:4], chain[4:], filler[4:]])
    assert len(np.unique(keys)) == len(keys) and (keys != 0).all()
    return keys


@functools.lru_cache(maxsize=None)
def chain_sets(row, family="one_sequence", variant="last"):
    """(chains, filler) of a row's chain case: one chain over 40 % of the
    table and random filler to 0.7 load; kt_part17: 200 chains of 256 keys
    among 60,000 random keys; kt_min with a wrapping chain: all 16 slots."""
    L, cap = KT_ROWS[row]["log2cap"], cap_of(row)
    make = (lambda n, s: one_sequence(L, n, s)) if family == "one_sequence" else (lambda n, s: wrapping(L, n, variant, s))
    if row == "kt_part17" and family == "wrapping":  # (2^17 slots: a handful of x have b1 = b2 or b1 = 0, so one chain each)
        return ([wrapping(L, 256, "b1_eq_b2"), wrapping(L, 256, "b1_zero")] +
                [wrapping(L, 256, "last", s) for s in range(198)]), key_pool(60_000)
    if row == "kt_part17":
        return [make(256, s) for s in range(200)], key_pool(60_000)
    if row == "kt_min" and family == "wrapping":
        return [make(cap, 0)], np.zeros(0, U64)
    n_chain = int(0.4 * cap)
    return [make(n_chain, 0)], key_pool(int(0.7 * cap) - n_chain)


def wrap_variants(row):
    """The wrap cases of a row: one per variant; kt_part17 has all three among its 200 chains."""
    return ("all",) if row == "kt_part17" else WRAP_VARIANTS


def chain_intervals(row, family="one_sequence", variant="last"):
    """The key sets of the three intervals -- half of every chain plus filler,
    then everything twice -- and each interval's chains."""
    chains, filler = chain_sets(row, family, variant)
    halves_ = [c[: len(c) // 2] for c in chains]
    half = hot_first(np.concatenate(halves_), filler)
    whole = hot_first(np.concatenate(chains), filler)
    return [half, whole, whole], [halves_, chains, chains]


def resident_after_flush(row, n_keys):
    """sa_flush's policy: the table is emptied once more than half of it (35 %
    of a binned table) is taken."""
    cap = cap_of(row)
    over = 20 * n_keys > 7 * cap if KT_ROWS[row]["path"] == "Binned" else 2 * n_keys > cap
    return 0 if over else n_keys


def full_chain_len(row, whole=False):
    return cap_of(row) if whole else max(int(0.4 * cap_of(row)), cap_of(row) // 4)


def full_keys(row, extra=0, whole=False):
    """table_capacity + extra distinct keys, 40 % of the table one chain and
    random filler; whole: all of them one chain, so that the table's last free
    slot is the last position of the sequence (max_probe - 1), and a lookup
    that stops one position early misses the key that took it."""
    if whole:
        return one_sequence(KT_ROWS[row]["log2cap"], cap_of(row) + extra, 0)
    n_chain = full_chain_len(row)
    return hot_first(one_sequence(KT_ROWS[row]["log2cap"], n_chain, 0), key_pool(cap_of(row) + extra - n_chain))


def halves_keys(row):
    return halves(KT_ROWS[row]["log2cap"], limit=int(0.7 * cap_of(row)))


def group_sets(row):
    """Two members' key sets for a flush through a group, all of one chain:
    member 0 holds exactly table_capacity keys of it (so one of them sits at
    the sequence's last position and no slot is empty), an eighth of them
    shared with member 1, which holds as many chain keys member 0 lacks."""
    L, cap = KT_ROWS[row]["log2cap"], cap_of(row)
    chain = one_sequence(L, cap + cap // 8, 0)
    return dict(only0=chain[: cap - cap // 8], both=chain[cap - cap // 8: cap], only1=chain[cap:], chain=chain)


def group_batch(rng, cfg, sets, w0=None):
    """A workload over the sets' union whose trace ids send every span of an
    only0 key to member 0 (trace_w1 even), of an only1 key to member 1, and
    the spans of a shared key alternately to both."""
    keys = hot_first(np.concatenate([sets["only0"][:4], sets["only1"], sets["only0"][4:]]), sets["both"])
    b = workload(rng, spans_for(len(keys)), cfg, keys, w0)
    w1 = b.trace_w1 & ~U64(1)
    w1[np.isin(b.key_hash, sets["only1"])] |= U64(1)
    sh = np.flatnonzero(np.isin(b.key_hash, sets["both"]))
    sh = sh[np.argsort(b.key_hash[sh], kind="stable")]
    ks = b.key_hash[sh]
    first = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    rank = np.arange(len(sh)) - np.repeat(first, np.diff(np.r_[first, len(sh)]))
    w1[sh] |= (rank & 1).astype(U64)
    b.trace_w1 = np.ascontiguousarray(w1)
    return b


def member_keys(batch, member, n=2):
    m = (batch.trace_w1 % U64(n)) == member
    k = np.unique(batch.key_hash[m])
    return k[k != 0]
