"""Host-side queries over one window's sketches (SURVEY.md rows a16-a17 and
Appendix C): count-min point queries, heavy hitters over the known ERROR
series, HLL estimates per service, and a simple per-window anomaly flag."""
from __future__ import annotations

from typing import Iterable, Sequence

import numpy as np

from .engine import hll_estimate

CMS_SEEDS = (0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB, 0xD6E8FEB86659FD93,
             0xA0761D6478BD642F, 0xE7037ED1A0B428DB, 0x8EBC6AF09C88C6E3, 0x589965CC75374CC3)
M64 = (1 << 64) - 1


def _splitmix64(x: int) -> int:
    z = (x + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def cms_query(cms: np.ndarray, key_hash: int) -> int:
    """min_j cms[j][splitmix64(key ^ seed_j) >> (64 - log2 w)]: an upper bound on
    the key's ERROR spans in the window (exact when no collision)."""
    d, w = cms.shape
    shift = 64 - (w.bit_length() - 1)
    return int(min(cms[j, _splitmix64(int(key_hash) ^ CMS_SEEDS[j]) >> shift] for j in range(d)))


def heavy_hitters(cms: np.ndarray, error_keys: Iterable[int], k: int = 10):
    """Top-k (key, estimate) over the host's ERROR series (status code 2 keys)."""
    est = [(int(key), cms_query(cms, key)) for key in error_keys]
    est = [e for e in est if e[1] > 0]
    est.sort(key=lambda e: (-e[1], e[0]))
    return est[:k]


def movers(cms_base: np.ndarray, cms_cur: np.ndarray, n_base: int, n_cur: int, keys: Iterable[int], k: int = 10,
           min_score: int = 1, fall: bool = False):
    """Top-k (key, score, baseline, current) of `keys` by the change of their
    ERROR spans per window from the baseline range (cms_base: the cells of
    its n_base windows summed) to the current one (cms_cur, n_cur): score =
    current * n_base - baseline * n_cur, negated when `fall` -- the difference
    of the per-window means times n_base * n_cur, so no division enters.  Rows
    with score >= max(min_score, 1), by score descending then key ascending."""
    rows = []
    for key in keys:
        b, c = cms_query(cms_base, key), cms_query(cms_cur, key)
        score = c * int(n_base) - b * int(n_cur)
        rows.append((int(key), -score if fall else score, b, c))
    rows = [r for r in rows if r[1] >= max(int(min_score), 1)]
    rows.sort(key=lambda r: (-r[1], r[0]))
    return rows[:k]


def error_onset(cms_windows, keys: Iterable[int], k: int = 10, min_count: int = 1, min_score: int = 1,
                fall: bool = False):
    """sa_window_error_onset over cms_windows [n][d][w], the cells of the
    range's windows in order: (rows, n_eligible, n_matched).  A key's sums S_r
    over the range give E = min_r S_r; it is eligible with E >= max(min_count,
    1).  For every split t in 1 .. n - 1, B(t) = min_r of the key's cells
    summed over windows 0 .. t - 1, A(t) = min_r of those summed over t .. n -
    1 (the two minima may come from different rows), D(t) = A(t) * t - B(t) *
    (n - t), negated when `fall`: movers' score of the two sides.  The best
    split has the largest D, the latest among equal ones.  A key matches when
    eligible with a best D >= max(min_score, 1).  rows: the first k matches by
    D descending then key ascending, each (key, t, D, B(t), A(t))."""
    x = np.asarray(cms_windows)
    n, d, w = x.shape
    shift = 64 - (w.bit_length() - 1)
    mc, ms = max(int(min_count), 1), max(int(min_score), 1)
    n_eligible, rows = 0, []
    for key in keys:
        cols = [_splitmix64(int(key) ^ CMS_SEEDS[r]) >> shift for r in range(d)]
        cell = [[int(x[j, r, cols[r]]) for j in range(n)] for r in range(d)]
        total = [sum(c) for c in cell]
        if min(total) < mc:
            continue
        n_eligible += 1
        best, prefix = None, [0] * d
        for t in range(1, n):
            prefix = [p + c[t - 1] for p, c in zip(prefix, cell)]
            b, a = min(prefix), min(s - p for s, p in zip(total, prefix))
            score = a * t - b * (n - t)
            score = -score if fall else score
            if best is None or score >= best[2]:
                best = (int(key), t, score, b, a)
        if best is not None and best[2] >= ms:
            rows.append(best)
    rows.sort(key=lambda r: (-r[2], r[0]))
    return rows[:k], n_eligible, len(rows)


def distinct_traces(hll: np.ndarray, p: int) -> np.ndarray:
    """[n_services] HLL estimates of distinct trace ids."""
    return np.array([hll_estimate(hll[s], p) for s in range(hll.shape[0])])


LAT_BINS = 256


def latency_bin(d_ns: int) -> int:
    """The latency histogram's bin of a duration in ns (include/spanagg.h,
    sa_latency_bin): bins 0..15 are 128 ns wide; from 2,048 ns up eight bins an
    octave; bin 255 has no upper bound."""
    q = int(d_ns) >> 7
    if q < 16:
        return q
    e = q.bit_length() - 1
    return min(LAT_BINS - 1, ((e - 3) << 3) + (q >> (e - 3)))


def latency_bin_bounds(b: int):
    """(lo, hi) of bin b in ns, inclusive (sa_latency_bin_bounds); hi of bin 255 is 2^64 - 1."""
    if not 0 <= b < LAT_BINS:
        raise ValueError("latency_bin_bounds: a bin in 0..255")
    if b < 16:
        return b << 7, (b << 7) + 127
    e, m = (b >> 3) + 2, b & 7
    return ((8 + m) << (e - 3)) << 7, M64 if b == LAT_BINS - 1 else (((9 + m) << (e - 3)) << 7) - 1


def latency_quantile_bin(hist, q_ppm: int) -> int:
    """The smallest bin whose cumulative count reaches r = max(1, ceil(count *
    q_ppm / 10^6)) -- sa_latency_result.q_bin; 0 for an empty histogram."""
    count = sum(int(c) for c in hist)
    if count == 0:
        return 0
    r = max(1, -(-count * int(q_ppm) // 1_000_000))
    run = 0
    for b, c in enumerate(hist):
        run += int(c)
        if run >= r:
            return b
    raise AssertionError("unreachable: r <= count")


def latency_movers(hist_base, hist_cur, q_ppm: Sequence[int], k: int, min_count: int = 1, min_shift: int = 1,
                   fall: bool = False):
    """sa_window_latency_movers over two [n_services][256] arrays, each a
    range's windows summed: (rows, n_eligible, n_matched).  A service is
    eligible with at least max(min_count, 1) spans in both; its shift is the
    bin of quantile q_ppm[0] in hist_cur minus that in hist_base (negated when
    `fall`); it matches with shift >= max(min_shift, 1).  rows: the first k
    matches by shift descending, then count_cur descending (clamped at 2^48 -
    1), then service ascending, each (service, shift, count_base, count_cur,
    q_bin_base, q_bin_cur) with the bins of every q_ppm as tuples."""
    mc, ms = max(int(min_count), 1), max(int(min_shift), 1)
    n_eligible, rows = 0, []
    for s, (hb, hc) in enumerate(zip(hist_base, hist_cur)):
        cb, cc = sum(int(c) for c in hb), sum(int(c) for c in hc)
        if cb < mc or cc < mc:
            continue
        n_eligible += 1
        qb = tuple(latency_quantile_bin(hb, p) for p in q_ppm)
        qc = tuple(latency_quantile_bin(hc, p) for p in q_ppm)
        shift = qb[0] - qc[0] if fall else qc[0] - qb[0]
        if shift >= ms:
            rows.append((s, shift, cb, cc, qb, qc))
    rows.sort(key=lambda r: (-r[1], -min(r[3], (1 << 48) - 1), r[0]))
    return rows[:k], n_eligible, len(rows)


def slo_counts(hist, threshold_bin: int):
    """sa_window_slo's counts of one summed 256-bin row: (total, slow), slow the
    spans in bins above threshold_bin -- the threshold's own bin counts as fast."""
    counts = [int(c) for c in hist]
    return sum(counts), sum(counts[int(threshold_bin) + 1:])


def slo_burning(total: int, slow: int, limit_ppm: int, min_count: int = 1) -> bool:
    """sa_window_slo's burn rule for one width: at least max(min_count, 1)
    spans, and slow * 10^6 > limit_ppm * total -- strictly, in integers."""
    total, slow = int(total), int(slow)
    return total >= max(int(min_count), 1) and slow * 1_000_000 > int(limit_ppm) * total


def latency_onset(pairs, min_count: int = 1, fall: bool = False):
    """sa_window_latency_onset's rule on one service's (total, slow) pairs, a
    window each: the split t in 1 .. len - 1 (before = windows 0 .. t - 1, after
    = the rest) with at least max(min_count, 1) spans on both sides and the
    largest D = S_after * N_before - S_before * N_after (negated when `fall`),
    the latest among equal D.  None without such a split, else (t, D,
    delta_ppm, N_before, S_before, N_after, S_after) with delta_ppm = S_after *
    10^6 // N_after - S_before * 10^6 // N_before (negated when `fall`).  The
    service matches when D > 0 and delta_ppm >= max(min_delta_ppm, 1)."""
    pairs = [(int(t), int(s)) for t, s in pairs]
    mc = max(int(min_count), 1)
    n, s = sum(p[0] for p in pairs), sum(p[1] for p in pairs)
    best, nb, sb = None, 0, 0
    for t in range(1, len(pairs)):
        nb, sb = nb + pairs[t - 1][0], sb + pairs[t - 1][1]
        na, sa = n - nb, s - sb
        if nb < mc or na < mc:
            continue
        d = sa * nb - sb * na
        d = -d if fall else d
        if best is None or d >= best[1]:
            delta = sa * 1_000_000 // na - sb * 1_000_000 // nb
            best = (t, d, -delta if fall else delta, nb, sb, na, sa)
    return best


def anomalous(series: Sequence[float], factor: float, min_base: float = 1.0) -> list:
    """Indices whose value exceeds `factor` x the series median (floor min_base)."""
    x = np.asarray(series, dtype=np.float64)
    base = max(float(np.median(x)), min_base)
    return [i for i, v in enumerate(x) if v > factor * base]
