"""Exponential-histogram geometries: the matrix rows over exp_max_size, the
counting geometry each must report, and a workload of named series families.

ROWS is shared by tests/test_expo_geometry_host.py (the generator against the
oracle, on the CPU) and tests/test_gpu_expo_geometry.py (the kernels on the
GPU).  The ingest side of a row follows geometry_util's rules (cap = the next
power of two >= 1.25 x key_capacity, lds = cap*41 + 24,704, the kernel
specialised for 2,048 slots and p = 14); the counting side is worked out here.

Counting kind.  1 slab counting: small table, at least one LDS entry fits.
2 cached-probe: SA_OPT_EXPO_CACHED.  3 the HBM passes: SA_OPT_EXPO_HBM.

Fold bins (slab counting only, 0 otherwise).  bin_slots = 16 up to max_size
2,048, 8 above; bins = cap / bin_slots: 128 and 256 at 2,048 slots, 32 and 64
at 512.

Entries, slab counting.  A counting workgroup has the LDS of a CU divided by
the ingest workgroups per CU (per_cu = grid_max / CUs), less 1 KiB:

  budget  = 163,840 / per_cu - 1,024            162,816 (one per CU), 80,896 (two)
  fixed   = cap*8 (slot words) + 256 (selection scratch) + 4,096*4 + 4 (tail
            records and their count) + bins*4 (run cursors) + 256*8 + 4 (the
            deferred long durations)
          = cap*8 + 18,696 + bins*4
  per     = ceil(max_size / 2) * 4              one entry's u16 pairs
  entries = min(cap, floor((budget - fixed) / per))

  2,048 slots (108,672 B of ingest LDS: one workgroup per CU), fixed 35,592
  with 128 bins, 36,104 with 256; budget - fixed = 127,224 and 126,712:
    max_size    2     3     5    159   161  1024  2048  2049  4095  4096
    per         4     8    12    320   324  2048  4096  4100  8192  8192
    quotient 31806 15903 10602 397.6 392.7  62.1  31.1  30.9  15.5  15.5
    entries   2048  2048  2048   397   392    62    31    30    15    15
  512 slots (45,696 B: one or two workgroups per CU, the device's registers
  decide), fixed 22,920 with 32 bins, 23,048 with 64:
    max_size              3        161       2049       4096
    one per CU   139,896/8 -> 512  431.8 -> 431  34.1 -> 34  17.1 -> 17
    two per CU    57,976/8 -> 512  178.9 -> 178  14.1 -> 14   7.1 -> 7
  (ENTRIES below; max_size 2, 3 and 5 come out at cap: every slot an entry.)

Entries, cached-probe: 256 halved while entries * max_size * 2 B > 64 KiB, not
below 4: 256 at 3; 256*129*2 = 66,048 > 65,536 -> 128 at 129; 8 at 4,096
(8*4,096*2 = 65,536).

The workload.  A row's series belong to families, all present in one batch:

  wide        log-uniform 1 ns .. 2^62 ns.  The series' ns sum is an exact u64
              that the comparison holds against a float64 sum, so a series
              keeps at most one span of 2^58 ns or more and eight of 2^52 ns or
              more per batch (the others are drawn again below 2^52).  The
              thick batch gives each series 1 ns, one unit (1 ms or 1 s: index
              -1, the last position of the circular bucket array at the scales
              a wide series ends at, 2,048 or more when max_size > 2,048) and
              2^61 ns.
  narrow-far  d0 + floor(u * eps * d0), d0 in {3 ns, 700 ns, 40 s, 3 h}.  The
              band is 0.75 * (max_size - 1) buckets wide at scale s_t (it
              touches at most max_size buckets there, so it settles at s_t or
              above): s_t = the smallest scale >= 9 at which the band is at
              most a quarter octave and every index of the band lies outside
              +-8,191 * 1.05.  (A band below 1 ns is the single value d0: scale
              20.)  Every batch holds both ends of each band.
  field-edge  the index field's edges at a settled scale.  One series cannot
              hold -8,193 and 8,192: its range is below max_size <= 4,096.  So
              per scale in (11, 12, 14) a low series holds -8,193, -8,192,
              -8,191 and a high series 8,190, 8,191, 8,192, each with the
              in-field values that pin the scale: the far end of a range of
              exactly max_size buckets (first bucket's lower half, last
              bucket's upper half: one scale up the range no longer fits) and
              its middle.  max_size 2 holds two adjacent indices per series:
              four series per scale.  Together they hold all six.
  single      one repeated value (scale 20, one bucket); only zeros; zeros and
              one positive value; end < start.  Two series each.
  bulk        the hot / cold series: a centre (1 us .. 10 s) and a width
              (0.05 .. 12 octaves) per series, 1 % zero, 1 % end < start.
              Roles: thin-hot (8), thick-hot (8), heavy (2), cold.  Half of
              the thick-hot series and one heavy one are `settled`: centres of
              0.1 .. 10 ms, widths 12, 6, 2, 0.5 and 6 octaves.

  thin batch   half its spans on the thin-hot series, 30 % on the cold series
               at even positions, 20 % on the other families; of each settled
               series three spans at either end of its band, no more.
  thick batch  half on the thick-hot series, a quarter on the two heavy series,
               the rest 8 : 1 : 1 on the cold series at odd positions, those at
               even positions and the other families.  The counting kernel
               takes its entries from the previous launch's counts, by their
               bit length.  The other thick-hot and heavy series and the odd
               cold ones are not in the thin batch: they hold no entry, and
               their records go the long way (the ingest kernel read scale 20).
               The settled series have their scale from the thin batch and, with
               six spans there (bit length 3), no entry either wherever at
               least `entries` series have eight spans or more (every slab row
               of up to 397 entries): their records are claimed on the counting
               loop's common path.  More than 90 % of a workgroup's share of
               4,608 spans are then tail records, past the 4,096 the buffer
               holds.  (Where every series holds an entry -- max_size 2, 3, 5,
               and 161 at 512 slots -- only the absent series' spans are: 57 %.)
               No probe tells a series' slot, and a workgroup's 4,096 records
               cannot fill 128 or more bins of 64 each: instead each heavy
               series alone puts an eighth of the workgroup's spans (> 500)
               into its own fold bin, whichever that is, and the run passes 64
               records.
  moving       launches A, B, C of narrow-far series only; B adds one value 41
               octaves or more away (3 ns and 700 ns x 2^45, 3 h -> 3 ns; 40 s
               has none inside 1 ns .. 2^62 ns) to two thirds of the series of
               those three d0: half of all.

About 1 % of every batch's spans have key 0; services, ends, traces and status
are geometry_util.make_batch's.
"""
import functools
import zlib

import numpy as np

import pyoracle
from geometry_util import THIN, key_pool, make_batch
from spanagg import Config, SpanBatch
from spanagg._lib import OPT_EXPO_CACHED, OPT_EXPO_HBM

SLAB, CACHED, HBM = 1, 2, 3
K_XT_CAP, K_XT_RUN = 4096, 64  # tail records per counting workgroup; records per fold-bin run
THICK_PER_WG = 4608
FIELD = 8191  # index records hold -8,192 .. 8,191
EDGE_SCALES = (11, 12, 14)
D0 = (3, 700, 40_000_000_000, 3 * 3_600_000_000_000)

# (slots, max_size, ingest workgroups per CU) -> LDS entries of slab counting (the docstring's arithmetic)
ENTRIES = {
    (2048, 2, 1): 2048, (2048, 3, 1): 2048, (2048, 5, 1): 2048, (2048, 159, 1): 397, (2048, 161, 1): 392,
    (2048, 1024, 1): 62, (2048, 2048, 1): 31, (2048, 2049, 1): 30, (2048, 4095, 1): 15, (2048, 4096, 1): 15,
    (512, 3, 1): 512, (512, 161, 1): 431, (512, 2049, 1): 34, (512, 4096, 1): 17,
    (512, 3, 2): 512, (512, 161, 2): 178, (512, 2049, 2): 14, (512, 4096, 2): 7,
}
CACHED_ENTRIES = {3: 256, 129: 128, 4096: 8}

_SPEC = dict(key_capacity=1500, n_windows=16)
_GENERIC = dict(key_capacity=400, hll_p=11, n_windows=16)


def _row(base, max_size, count, **cfg):
    cfg = dict(base, exp_max_size=max_size, **cfg)
    spec = cfg["key_capacity"] == 1500
    hbm = count == HBM
    return dict(cfg=cfg, max_size=max_size, count=count, cap=2048 if spec else 512,
                path="ExpoHbm" if hbm else "ExpoSmall",
                kernel="bounds16" if hbm else "expo_specialised" if spec else "expo_generic",
                lb=(13, 2048) if spec else (10, 2048),  # 16*64*2^14 = 2^24 >> 13; 16*64*2^11 = 2^21 >> 10
                lds=0 if hbm else (2048 if spec else 512) * 41 + 24_704)


ROWS = {f"spec_{m}": _row(_SPEC, m, SLAB) for m in (2, 3, 5, 159, 161, 1024, 2048, 2049, 4095, 4096)}
ROWS.update({f"generic_{m}": _row(_GENERIC, m, SLAB, **({"unit": "s"} if m == 2049 else {}))
             for m in (3, 161, 2049, 4096)})
ROWS.update({f"cached_{m}": _row(_SPEC, m, CACHED, options=OPT_EXPO_CACHED) for m in (3, 129, 4096)})
ROWS.update({f"hbm_{m}": _row(_SPEC, m, HBM, options=OPT_EXPO_HBM) for m in (3, 2049, 4096)})


def config_of(row) -> Config:
    return Config(**ROWS[row]["cfg"])


def slab_entries(cap, max_size, per_cu) -> int:
    """expo_slab_entries' formula (the module docstring)."""
    bins = cap // (16 if max_size <= 2048 else 8)
    fixed = cap * 8 + 256 + K_XT_CAP * 4 + 4 + bins * 4 + 256 * 8 + 4
    return min(cap, (163_840 // per_cu - 1024 - fixed) // ((max_size + 1) // 2 * 4))


def expected_counting(row, per_cu) -> dict:
    """The counting fields of debug_geometry() a row must report on a device
    that runs per_cu ingest workgroups per CU."""
    r = ROWS[row]
    M, cap = r["max_size"], r["cap"]
    if r["count"] == SLAB:
        bs = 16 if M <= 2048 else 8
        return dict(expo_count=SLAB, expo_entries=ENTRIES[cap, M, per_cu], expo_bin_slots=bs, expo_bins=cap // bs)
    return dict(expo_count=r["count"], expo_entries=CACHED_ENTRIES[M] if r["count"] == CACHED else 0,
                expo_bin_slots=0, expo_bins=0)


def assert_counting_geometry(e, row, cus) -> dict:
    """Engine.debug_geometry() against the row: the ingest kernel as
    geometry_util.assert_geometry checks it, then the counting pass."""
    r, g = ROWS[row], e.debug_geometry()
    assert (g["path"], g["kernel"], g["log2cap"]) == (r["path"], r["kernel"], r["cap"].bit_length() - 1), g
    assert (g["lb_shift"], g["lb_n"]) == r["lb"], g
    assert g["error_table"] == (r["count"] != HBM) and g["lds_bytes"] == r["lds"], g  # 16 * cap < 65,535
    assert g["block"] == (256 if r["count"] == HBM else 1024), g
    assert g["grid_max"] > 0 and g["grid_max"] % cus == 0, (g, cus)
    per_cu = g["grid_max"] // cus
    if r["count"] != HBM:
        assert per_cu == 1 if r["cap"] == 2048 else per_cu in (1, 2), g
    want = expected_counting(row, per_cu)
    assert {k: g[k] for k in want} == want, (g, want)
    if r["count"] == SLAB:
        assert g["expo_entries"] > 0
        if r["max_size"] <= 5:
            assert g["expo_entries"] == r["cap"]
    return g


def thick_size(row, grid_max, cus) -> int:
    """grid_max * 4,608 + 17 spans for the counting workgroups of a small
    table, one per ingest workgroup.  An HBM table has no counting workgroups
    (its grid_max is the sketch kernel's, eight 256-thread workgroups per CU):
    its batch is the one-workgroup-per-CU size."""
    return (cus if ROWS[row]["count"] == HBM else grid_max) * THICK_PER_WG + 17


# ---- the families ------------------------------------------------------------------------------------------------

def duration_at(index, scale, div, half=None) -> int:
    """A duration in ns whose oracle bucket index at `scale` is `index`
    (half: 0 / 1 = in the lower / upper half of the bucket, by the index one
    scale up)."""
    def ok(d):
        if d < 1 or pyoracle.expo_index(d / div, scale) != index:
            return False
        return half is None or pyoracle.expo_index(d / div, scale + 1) == 2 * index + half
    frac = 0.5 if half is None else 0.25 + 0.5 * half
    guess = int(round(div * 2.0 ** ((index + frac) / 2.0 ** scale)))
    for k in range(0, 64):
        for d in (guess + k, guess - k):
            if ok(d):
                return d
    raise ValueError(f"no integer ns duration at index {index}, scale {scale}")


def edge_index_sets(max_size):
    """The index sets of the field-edge series at one scale: (targets, pins)."""
    M = max_size
    if M == 2:
        return [([a, a + 1], []) for a in (-FIELD - 2, -FIELD - 1, FIELD - 1, FIELD)]
    lo, hi = -FIELD - 2, FIELD + 1
    return [([lo, lo + 1, lo + 2], [lo + M - 1, lo + M // 2]), ([hi - 2, hi - 1, hi], [hi - (M - 1), hi - M // 2])]


def narrow_band(d0, max_size, div):
    """(s_t, span): the band [d0, d0 + span] ns and the scale it settles at."""
    M, l2 = max_size, np.log2(d0 / div)
    for s in range(9, 21):
        width = 0.75 * (M - 1) / 2.0 ** s  # octaves
        far = abs(l2) * 2.0 ** s - (0.75 * M if l2 < 0 else 0)
        if width <= 0.25 and far >= 1.05 * (FIELD + 1):
            return s, int(d0 * (2.0 ** width - 1))
    return 20, 0


class Plan:
    """A row's series: their ids by family and each series' parameters, the
    same for every batch of the row."""

    def __init__(self, row):
        r = ROWS[row]
        self.row, self.cfg, self.M = row, config_of(row), r["max_size"]
        self.div = 1e9 if self.cfg.unit == "s" else 1e6
        big = r["cfg"]["key_capacity"] == 1500
        n_wide, n_per, n_bulk = (16, 12, 1400) if big else (8, 6, 340)
        edges = [(s, t, p) for s in EDGE_SCALES for t, p in edge_index_sets(self.M)]
        n = n_wide + 4 * n_per + len(edges) + 8 + n_bulk
        assert n <= r["cfg"]["key_capacity"]
        ids = iter(np.split(key_pool(n), np.cumsum([n_wide, 4 * n_per, len(edges), 8])))
        self.wide, self.narrow, self.edge, self.single, self.bulk = (next(ids) for _ in range(5))
        rng = np.random.default_rng(zlib.crc32(row.encode()))
        # narrow-far: n_per series per d0
        self.narrow_d0 = np.repeat(np.array(D0, dtype=np.uint64), n_per)
        self.narrow_span = np.repeat(np.array([narrow_band(d, self.M, self.div)[1] for d in D0], dtype=np.uint64), n_per)
        # launch B's far value: two thirds of the series of 3 ns, 700 ns and 3 h
        far = {3: 3 << 45, 700: 700 << 45, D0[3]: 3}
        self.narrow_far = np.array([far.get(int(d), 0) if k % n_per < 2 * n_per // 3 else 0
                                    for k, d in enumerate(self.narrow_d0)], dtype=np.uint64)
        # field-edge: the value list of each series
        self.edge_scale = [s for s, _, _ in edges]
        self.edge_targets = [t for _, t, _ in edges]
        self.edge_values = []
        for s, t, p in edges:
            idx = sorted(set(t + p))
            vals = [duration_at(i, s, self.div, half=0 if i == idx[0] else 1 if i == idx[-1] else None) for i in idx]
            self.edge_values.append(np.array(vals, dtype=np.uint64))
        # bulk: centre and width per series
        self.bulk_centre = 10.0 ** rng.uniform(3, 10, n_bulk)
        self.bulk_width = rng.choice([0.05, 0.5, 2.0, 6.0, 12.0], n_bulk)
        b = self.bulk
        self.thin_hot, self.thick_hot, self.heavy = b[:8], b[8:16], b[16:18]
        # the settled half of the thick-hot and heavy series: around 1 ms, each width once
        self.settled = np.array([8, 9, 10, 11, 16])
        self.bulk_centre[self.settled] = 10.0 ** rng.uniform(5, 7, len(self.settled))
        self.bulk_width[self.settled] = [12.0, 6.0, 2.0, 0.5, 6.0]
        self.cold_even, self.cold_odd = b[18::2], b[19::2]
        self.special = np.concatenate([self.wide, self.narrow, self.edge, self.single])

    # the durations of spans of one family; k = each span's series within the family
    def _wide(self, rng, k, thick):
        d = np.floor(2.0 ** rng.uniform(0, 62, len(k))).astype(np.uint64)
        for floor_, limit in ((1 << 58, 0 if thick else 1), (1 << 52, 8)):
            again = _beyond(k, d >= floor_, limit)
            d[again] = np.floor(2.0 ** rng.uniform(0, 52, len(again))).astype(np.uint64)
        return np.maximum(d, 1)

    def _narrow(self, rng, k):
        return self.narrow_d0[k] + (rng.random(len(k)) * (self.narrow_span[k] + np.uint64(1)).astype(np.float64)
                                    ).astype(np.uint64)

    def _edge(self, rng, k):
        d = np.zeros(len(k), dtype=np.uint64)
        for j, vals in enumerate(self.edge_values):
            m = k == j
            d[m] = vals[rng.integers(0, len(vals), int(m.sum()))]
        return d

    def _single(self, rng, k):
        """(durations, end < start) -- series 0, 1 one value; 2, 3 zeros; 4, 5
        zeros and one positive value; 6, 7 end < start."""
        d = np.zeros(len(k), dtype=np.uint64)
        d[k < 2] = 7_777_777
        pos = (k >= 4) & (k < 6) & (rng.random(len(k)) < 0.3)
        d[pos] = 123_456
        return d, k >= 6

    def _bulk(self, rng, k):
        """(durations, end < start)"""
        d = self.bulk_centre[k] * 2.0 ** (self.bulk_width[k] * (rng.random(len(k)) - 0.5))
        d = np.maximum(d, 1.0).astype(np.uint64)
        u = rng.random(len(k))
        d[u < 0.01] = 0
        return d, (u >= 0.01) & (u < 0.02)

    def _spans(self, rng, fam, k, thick=False):
        """(keys, durations, end < start) of spans of series k of one family."""
        back = np.zeros(len(k), dtype=bool)
        if fam == "wide":
            d = self._wide(rng, k, thick)
        elif fam == "narrow":
            d = self._narrow(rng, k)
        elif fam == "edge":
            d = self._edge(rng, k)
        elif fam == "single":
            d, back = self._single(rng, k)
        else:
            d, back = self._bulk(rng, k)
        return getattr(self, fam)[k], d, back

    def _special_spans(self, rng, n, thick):
        """n spans over the four special families, each series alike."""
        sizes = [len(self.wide), len(self.narrow), len(self.edge), len(self.single)]
        which = rng.integers(0, sum(sizes), n)
        off = np.concatenate([[0], np.cumsum(sizes)])
        parts = []
        for j, fam in enumerate(("wide", "narrow", "edge", "single")):
            k = which[(which >= off[j]) & (which < off[j + 1])] - off[j]
            parts.append(self._spans(rng, fam, k, thick))
        return parts

    def _sure(self, thick, narrow_only=False):
        """The spans a batch holds for sure: both ends of every narrow band;
        every value of every field-edge series; a positive value for single
        series 4 and 5; in the thin batch the settled series' six spans; in the thick batch each wide series' 1 ns, one unit, 2^61 ns."""
        key = [self.narrow, self.narrow]
        dur = [self.narrow_d0, self.narrow_d0 + self.narrow_span]
        if not narrow_only:
            for j, vals in enumerate(self.edge_values):
                key.append(np.full(len(vals), self.edge[j], dtype=np.uint64))
                dur.append(vals)
            key.append(self.single[4:6])
            dur.append(np.full(2, 123_456, dtype=np.uint64))
            if not thick:  # both ends of the settled series' bands, three spans each
                for sign in (-0.5, 0.5):
                    key.append(np.repeat(self.bulk[self.settled], 3))
                    d = self.bulk_centre[self.settled] * 2.0 ** (sign * self.bulk_width[self.settled])
                    dur.append(np.repeat(np.maximum(d, 1.0).astype(np.uint64), 3))
            if thick:
                for v in (1, int(self.div), 1 << 61):
                    key.append(self.wide)
                    dur.append(np.full(len(self.wide), v, dtype=np.uint64))
        key, dur = np.concatenate(key), np.concatenate(dur).astype(np.uint64)
        return key, dur, np.zeros(len(key), dtype=bool)

    def _batch(self, rng, n, parts, sure) -> SpanBatch:
        """n spans: `sure` plus the random `parts` (cut to n; ~1 % of them key
        0), shuffled, on make_batch's services, ends, traces and status."""
        key, dur, back = (np.concatenate([p[i] for p in parts]) for i in range(3))
        m = n - len(sure[0])
        assert 0 < m <= len(key), (n, m, len(key))
        pick = rng.permutation(len(key))[:m]
        key, dur, back = key[pick], dur[pick], back[pick]
        key[rng.random(m) < 0.01] = 0
        key, dur, back = (np.concatenate([a, b]) for a, b in zip((key, dur, back), sure))
        order = rng.permutation(n)
        key, dur, back = key[order], dur[order].astype(np.uint64), back[order]
        base = make_batch(rng, n, self.cfg, 16)
        start = base.end_ns - dur  # (ends lie past 2^62 ns: geometry_util.ring_start)
        start[back] = base.end_ns[back] + rng.integers(1, 1_000_000, int(back.sum()), dtype=np.uint64)
        return SpanBatch(key, start, base.end_ns, base.trace_w0, base.trace_w1, base.meta)

    def _bulk_spans(self, rng, ids_of, n):
        """n spans uniform over the bulk series at positions ids_of (in self.bulk)."""
        return self._spans(rng, "bulk", ids_of[rng.integers(0, len(ids_of), n)])

    def thin(self, rng, n=THIN) -> SpanBatch:
        nb = len(self.bulk)
        parts = [self._bulk_spans(rng, np.arange(0, 8), n // 2),
                 self._bulk_spans(rng, np.arange(18, nb, 2), 3 * n // 10)]
        parts += self._special_spans(rng, n - n // 2 - 3 * n // 10 + 64, thick=False)
        return self._batch(rng, n, parts, self._sure(thick=False))

    def thick(self, rng, n) -> SpanBatch:
        nb, rest = len(self.bulk), n - n // 2 - n // 4
        parts = [self._bulk_spans(rng, np.arange(8, 16), n // 2),
                 self._bulk_spans(rng, np.arange(16, 18), n // 4),
                 self._bulk_spans(rng, np.arange(19, nb, 2), 8 * rest // 10),
                 self._bulk_spans(rng, np.arange(18, nb, 2), rest // 10)]
        parts += self._special_spans(rng, rest - 8 * rest // 10 - rest // 10 + 64, thick=True)
        return self._batch(rng, n, parts, self._sure(thick=True))

    def moving(self, rng, n=THIN):
        """Launches A, B, C: narrow-far series only; B with the far values."""
        out = []
        for launch in range(3):
            k = rng.integers(0, len(self.narrow), n + 64)
            sure = self._sure(False, narrow_only=True)
            if launch == 1:
                has = self.narrow_far != 0
                sure = tuple(np.concatenate([a, b]) for a, b in
                             zip(sure, (self.narrow[has], self.narrow_far[has], np.zeros(int(has.sum()), dtype=bool))))
            out.append(self._batch(rng, n, [self._spans(rng, "narrow", k)], sure))
        return out


def _beyond(k, mask, limit) -> np.ndarray:
    """The positions of the spans of `mask` past the first `limit` of their series."""
    idx = np.flatnonzero(mask)
    order = np.argsort(k[idx], kind="stable")
    ks = k[idx][order]
    if len(ks) == 0:
        return idx
    first = np.concatenate([[0], np.flatnonzero(ks[1:] != ks[:-1]) + 1])
    rank = np.arange(len(ks)) - np.repeat(first, np.diff(np.concatenate([first, [len(ks)]])))
    return idx[order][rank >= limit]


@functools.lru_cache(maxsize=None)
def plan_of(row) -> Plan:
    return Plan(row)


def rng_of(row, what):
    return np.random.default_rng(zlib.crc32(f"{row} {what}".encode()))
