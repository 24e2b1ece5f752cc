"""sa_window_latency_onset: the numpy restatement the GPU tests compare with,
built on tests/latency_util.py and tests/slo_util.py (whose workloads most of
these are), and the workloads both the GPU tests and the host tests
(tests/test_window_onset_host.py, which holds spanagg.sketch.latency_onset
against it) run.

  thresholds   every service's bin: sa_latency_bin of the given threshold, or
               the pooled quantile's bin of its rows summed over the range
  pairs        per service and window of the range (total, slow), slow the
               spans in bins above the service's bin
  splits       per service the eligible split t in 1 .. n_cov - 1 (both sides
               hold max(min_count, 1) spans) with the largest D = S_a N_b - S_b
               N_a (negated under fall), the latest among equal D -- D in
               Python integers, so the 2^88 products are exact -- and
               delta_ppm = S_a 10^6 // N_a - S_b 10^6 // N_b
  select       matched = eligible, D > 0 and delta_ppm >= max(min_delta_ppm,
               1); ordered by delta_ppm descending, min(N, 2^44 - 1)
               descending, service ascending; the first k

The `wrong` switch builds the references that make a known mistake: "ge_bin"
(the threshold's own bin counted slow), "first_tie" (the earliest split wins a
tie), "d_i64" (D wrapped to 64 bits), "one_sided_min" (only N_b held against
min_count), "edge_split" (t = 0 and t = n_cov allowed, the empty side
unchecked and its share 0), "unfloored" (delta_ppm from one division of D).
The host tests show that the workloads tell each from the right one.

A ring case is its configuration, the (ring base, batch) steps that fill the
ring, the per-window histograms after them (computed once, shared and never
changed) and the calls made against it; a probe case is pairs [n_sel][n_cov]
[2] and calls, for sa_onset_probe.
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import latency_util as lu
import slo_util as su
from geometry_util import ring_start
from spanagg import TOP_MAX_K

U = np.uint64
WRONG = ("ge_bin", "first_tie", "d_i64", "one_sided_min", "edge_split", "unfloored")
COUNT_TOP = (1 << 44) - 1
FIELDS = ("services", "onset_window", "delta_ppm", "threshold_bin", "effective_ns", "total_before", "slow_before",
          "total_after", "slow_after")
SCALARS = ("first", "last", "fall", "q_ppm", "min_count", "n_services", "n_eligible", "n_matched", "spans")


@dataclasses.dataclass(frozen=True)
class Call:
    first: int
    last: int
    k: int = 10
    quantile: float = 0.95         # the pooled threshold's (thresholds is None)
    thresholds: tuple = None       # one a service: the given thresholds
    min_count: int = 1
    min_delta_ppm: int = 1
    fall: bool = False

    def args(self):
        """As Engine.window_latency_onset takes them."""
        return (self.first, self.last, self.k, self.quantile, self.thresholds, self.min_count, self.min_delta_ppm,
                self.fall)

    @property
    def q_ppm(self):
        return 0 if self.thresholds is not None else int(round(self.quantile * 1e6))


def thresholds(ref, cfg, call) -> np.ndarray:
    """[n_services] the bin every service is cut at."""
    if call.thresholds is not None:
        thr = np.asarray(call.thresholds, dtype=np.uint64)
        assert thr.shape == (cfg.n_services,)
        return lu.bins_of(thr)
    pooled = lu.ring_hists(ref, cfg, call.first, call.last).sum(axis=0, dtype=np.uint64)
    return lu.quantile_bins(pooled, [call.q_ppm])[1][:, 0].astype(np.int64)


def pairs(ref, cfg, call, tb, wrong=None) -> np.ndarray:
    """[n_services][n_cov][2] u64: (total, slow) of every service and window of the range."""
    h = lu.ring_hists(ref, cfg, call.first, call.last)  # [n_cov][S][256]
    bins = np.arange(lu.BINS)
    above = bins[None, :] >= tb[:, None] if wrong == "ge_bin" else bins[None, :] > tb[:, None]
    tot = h.sum(axis=-1, dtype=np.uint64)
    slow = np.where(above[None], h, U(0)).sum(axis=-1, dtype=np.uint64)
    return np.ascontiguousarray(np.stack([tot, slow], axis=-1).transpose(1, 0, 2))


def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >> 63 else v


def split(p, min_count=1, fall=False, wrong=None):
    """One service's pairs [n_cov][2] -> None without an eligible split, else
    (t, D, delta_ppm, N_b, S_b, N_a, S_a): the rule above, on Python integers."""
    tot, slow = [int(v) for v in p[:, 0]], [int(v) for v in p[:, 1]]
    n_cov, mc = len(tot), max(int(min_count), 1)
    cn, cs = np.concatenate([[0], np.cumsum(tot, dtype=object)]), np.concatenate([[0], np.cumsum(slow, dtype=object)])
    N, S = int(cn[-1]), int(cs[-1])
    best = None
    for t in range(0, n_cov + 1) if wrong == "edge_split" else range(1, n_cov):
        nb, sb = int(cn[t]), int(cs[t])
        na, sa = N - nb, S - sb
        if wrong == "edge_split" and t in (0, n_cov):
            if max(nb, na) < mc:
                continue
        elif nb < mc or (na < mc and wrong != "one_sided_min"):
            continue
        d = sa * nb - sb * na
        if wrong == "d_i64":
            d = _i64(_i64(sa * nb) - _i64(sb * na))
        d = -d if fall else d
        if best is None or d > best[1] or (d == best[1] and wrong != "first_tie"):
            if wrong == "unfloored":
                delta = (sa * nb - sb * na) * 1_000_000 // (na * nb) if na and nb else 0
            else:
                delta = (sa * 1_000_000 // na if na else 0) - (sb * 1_000_000 // nb if nb else 0)
            best = (t, d, -delta if fall else delta, nb, sb, na, sa)
    return best


def scan(p, k, min_count=1, min_delta_ppm=1, fall=False, wrong=None, first=0):
    """pairs [n_sel][n_cov][2] -> the call's answer as a namespace of FIELDS
    (threshold_bin and effective_ns left to the caller) and counters."""
    p = np.asarray(p, dtype=np.uint64)
    n_sel, rows, n_eligible, spans = p.shape[0], [], 0, 0
    for s in range(n_sel):
        N = int(p[s, :, 0].sum(dtype=object)) if p.shape[1] else 0
        spans += N
        b = split(p[s], min_count, fall, wrong)
        if b is None:
            continue
        n_eligible += 1
        if b[1] > 0 and b[2] >= max(int(min_delta_ppm), 1):
            rows.append((s, N) + b)
    rows.sort(key=lambda r: (-r[4], -min(r[1], COUNT_TOP), r[0]))
    top = rows[:k]
    col = lambda j, dt: np.array([r[j] for r in top], dtype=dt)
    return SimpleNamespace(
        services=col(0, np.uint32), onset_window=(col(2, np.uint64) + U(first)).astype(np.uint64),
        delta_ppm=col(4, np.int32), total_before=col(5, np.uint64), slow_before=col(6, np.uint64),
        total_after=col(7, np.uint64), slow_after=col(8, np.uint64), n_services=n_sel, n_eligible=n_eligible,
        n_matched=len(rows), spans=spans, splits=[r[2] for r in top], d=[r[3] for r in top])


def expected(ref, cfg, call, wrong=None):
    """What window_latency_onset(*call.args()) must return."""
    tb = thresholds(ref, cfg, call)
    w = scan(pairs(ref, cfg, call, tb, wrong), call.k, call.min_count, call.min_delta_ppm, call.fall, wrong, call.first)
    w.threshold_bin = tb[w.services.astype(np.int64)].astype(np.uint8)
    w.effective_ns = lu.BIN_HI[w.threshold_bin.astype(np.int64)]
    w.first, w.last, w.fall, w.q_ppm, w.min_count = call.first, call.last, call.fall, call.q_ppm, max(call.min_count, 1)
    return w


def expected_probe(p, k, min_count=1, min_delta_ppm=1, fall=False, wrong=None):
    """What onset_probe(p, k, min_count, min_delta_ppm, fall) must return."""
    w = scan(p, k, min_count, min_delta_ppm, fall, wrong)
    n = len(w.services)
    w.threshold_bin, w.effective_ns = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
    w.first, w.last, w.fall, w.q_ppm, w.min_count = 0, np.asarray(p).shape[1] - 1, fall, 0, max(min_count, 1)
    return w


def assert_onset(res, want, what=""):
    for f in SCALARS:
        assert getattr(res, f) == getattr(want, f), (f, getattr(res, f), getattr(want, f), what)
    for f in FIELDS:
        a, b = getattr(res, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (f, a, b, what)


def same(a, b, what=""):
    """Two results field by field."""
    assert_onset(a, b, what)


# ---------------------------------------------------------------- ring cases

def _case(cfg, steps, calls, **more):
    return SimpleNamespace(cfg=cfg, steps=steps, ref=lu.window_hists(cfg, steps), calls=calls, **more)


def _of_slo(name, calls, **more):
    """slo_util's workload `name` (its reference shared, never changed) with this query's calls."""
    c = su.case(name)
    return SimpleNamespace(cfg=c.cfg, steps=c.steps, ref=c.ref, calls=calls, **more)


def _shifted(cfg, w0, n_windows, rng, per_cell, shifts):
    """Spans of windows w0 .. w0 + n_windows - 1: per (window, service) up to 2
    * per_cell of them (some cells empty), durations log-uniform over 1 us ..
    100 ms; service s's durations are multiplied by shifts[s][1] from window
    index shifts[s][0] on."""
    S = cfg.n_services
    cnt = rng.integers(0, 2 * per_cell + 1, (n_windows, S))
    cnt[rng.random((n_windows, S)) < 0.1] = 0
    win, svc = np.divmod(np.repeat(np.arange(n_windows * S), cnt.reshape(-1)), S)
    d = np.exp(rng.uniform(np.log(1e3), np.log(1e8), len(win)))
    for s, (at, factor) in shifts.items():
        m = (svc == s) & (win >= at)
        d[m] *= factor
    return _spans(cfg, w0 + win, svc, d)


def _spans(cfg, windows, services, durations):
    """One span a (window, service, duration) triple, ending inside its window."""
    from spanagg import SpanBatch, pack_meta
    n = len(durations)
    end = np.asarray(windows, dtype=np.uint64) * U(cfg.window_ns) + U(5)
    k = np.arange(1, n + 1, dtype=np.uint64)
    return SpanBatch(k, end - np.asarray(durations, dtype=np.uint64), end, k, k,
                     pack_meta(np.asarray(services), np.zeros(n), np.zeros(n)))


def _lengths():
    """A 128-window ring of 3 services whose latency shifts at windows 40 (up),
    70 (down) and never: ranges of 1, 2, 64, 65, 127 and 128 windows -- no
    split, one, the scan's carry across one step, a last step that is not full
    -- under both thresholds."""
    cfg = su._cfg(3, 128)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"onset_lengths"))
    batch = _shifted(cfg, w0, 128, rng, 60, {0: (40, 8.0), 1: (70, 0.2)})
    thr = (250_000, int(lu.BIN_HI[150]), 1_000_000)
    calls = []
    for a, n_cov in ((w0 + 5, 1), (w0 + 39, 2), (w0 + 10, 64), (w0 + 10, 65), (w0 + 1, 127), (w0, 128)):
        calls.append(Call(a, a + n_cov - 1, 3, 0.9, None, 20))
        calls.append(Call(a, a + n_cov - 1, 3, 0.0, thr, 20))
    calls.append(Call(w0, w0 + 127, 3, 0.9, None, 20, 1, True))
    return _case(cfg, [(w0, batch)], calls, w0=w0)


def _moved():
    """slo_util's moved ring (32 windows moved by 13: the slots wrap), the whole
    ring and a part of it, both thresholds, rise and fall."""
    base = su.case("moved").base
    thr = (1_000_000,)
    calls = [Call(base, base + 31, 5, 0.9), Call(base, base + 31, 5, 0.0, thr), Call(base, base + 31, 5, 0.9, None, 1, 1, True),
             Call(base, base + 31, 5, 0.0, thr, 3_000, 1, True), Call(base + 4, base + 20, 1, 0.5, None, 3_000)]
    return _of_slo("moved", calls, base=base)


def _services(S):
    """slo_util's S services on 8 windows: k of 1, 10 and SA_TOP_MAX_K -- the
    gather, the grid, n_matched above and below k."""
    c = su.case(f"services{S}")
    thr = c.calls[0].thresholds
    calls = [Call(c.w0, c.w0 + 7, 1, 0.9), Call(c.w0, c.w0 + 7, 10, 0.0, thr), Call(c.w0, c.w0 + 7, TOP_MAX_K, 0.75),
             Call(c.w0, c.w0 + 7, TOP_MAX_K, 0.0, thr, 5, 20_000, True)]
    return _of_slo(f"services{S}", calls, w0=c.w0)


def every_bin_ppm(b):
    """The q_ppm whose pooled bin is b on _every_bin's rows: 512 spans, 257 + b
    of them in bins 0..b, so the rank must be 257 + b."""
    return (256 + b) * 1_000_000 // 512 + 1


EVERY_BIN_POOLED = (0, 1, 2) + tuple(b for l in range(64) for b in (4 * l + 3, 4 * l + 4) if b < 256)


def _every_bin():
    """slo_util's every_bin (256 services, one span in each of the 256 bins of
    window w0 + 1) behind a window w0 that holds the same spans, all in bin 0.
    Given thresholds: service s's at the lower bound of bin s -- one split,
    (256, 0) before and (256, 255 - s) after.  Pooled: every service's row is
    257 spans in bin 0 and one in every other bin, so quantile every_bin_ppm(b)
    cuts every service at bin b -- a call a lane boundary."""
    c = su.case("every_bin")
    svc = np.repeat(np.arange(256), 256)
    steps = [(c.w0, _spans(c.cfg, np.full(len(svc), c.w0), svc, np.zeros(len(svc))))] + list(c.steps)
    thr = tuple(int(v) for v in su.BIN_LO)
    calls = [Call(c.w0, c.w0 + 1, 256, 0.0, thr)]
    calls += [Call(c.w0, c.w0 + 1, 256, every_bin_ppm(b) / 1e6) for b in EVERY_BIN_POOLED]
    return _case(c.cfg, steps, calls, w0=c.w0)


CRAFTED_PAIRS = ((100, 0), (100, 1), (0, 0), (100, 40), (100, 50), (100, 45))


def _crafted(seq):
    """One service, threshold at BIN_HI[100] (a bin's upper bound: exact),
    window j holding seq[j] = (total, slow)."""
    cfg = su._cfg(1, 8)
    w0 = ring_start(cfg)
    win, d = [], []
    for j, (tot, slow) in enumerate(seq):
        win += [w0 + j] * tot
        d += [su.CRAFTED_FAST] * (tot - slow) + [su.CRAFTED_SLOW] * slow
    thr = (su.CRAFTED_THRESHOLD,)
    n = len(seq)
    one = lambda **kw: Call(w0, w0 + n - 1, 1, 0.0, thr, **kw)
    calls = [one(), one(min_count=200), one(min_count=201), one(fall=True), Call(w0, w0, 1, 0.0, thr),
             one(min_delta_ppm=445_000), one(min_delta_ppm=445_001), one(min_delta_ppm=1_000_001)]
    return _case(cfg, [(w0, _spans(cfg, win, np.zeros(len(d)), d))], calls, w0=w0)


_BUILD = {"lengths": _lengths, "moved": _moved, "every_bin": _every_bin,
          "crafted": functools.partial(_crafted, CRAFTED_PAIRS),
          "crafted_rev": functools.partial(_crafted, CRAFTED_PAIRS[::-1]),
          "crafted_flat": functools.partial(_crafted, ((10, 1),) * 6),
          **{f"services{S}": functools.partial(_services, S) for S in (1, 64, 129, 1000)}}
CASES = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def want(name, j):
    """expected() of call j of case `name`, computed once."""
    c = case(name)
    return expected(c.ref, c.cfg, c.calls[j])


# ---------------------------------------------------------------- probe cases

@dataclasses.dataclass(frozen=True)
class ProbeCall:
    k: int = 10
    min_count: int = 1
    min_delta_ppm: int = 1
    fall: bool = False

    def args(self):
        return (self.k, self.min_count, self.min_delta_ppm, self.fall)


def _big():
    """Six services on seven windows with counts near 2^43 -- a service's total
    stays below 2^44 -- so the products pass 2^86: service 0's two candidate
    splits differ in D by less than 2^64 wraps away, the others are drawn."""
    rng = np.random.default_rng(zlib.crc32(b"onset_big"))
    p = np.zeros((6, 7, 2), np.uint64)
    # service 0: a step from 1 % to 51 % slow at window 4, and a head-fake at window 2
    tot = [1 << 41] * 7
    slow = [tot[0] // 100, tot[0] // 100, tot[0] // 50, tot[0] // 100, tot[0] // 2, tot[0] // 2 + 7, tot[0] // 2]
    p[0, :, 0], p[0, :, 1] = tot, slow
    for s in range(1, 6):
        t = rng.integers(1 << 39, (1 << 44) // 7, 7, dtype=np.uint64)
        share = np.where(np.arange(7) >= rng.integers(1, 7), rng.uniform(0.3, 0.9), rng.uniform(0.0, 0.3))
        p[s, :, 0], p[s, :, 1] = t, (t.astype(np.float64) * share).astype(np.uint64)
    p[5, :, 0] = (1 << 44) // 7 - 1  # the busiest row: just below 2^44 in all
    p[5, :, 1] = p[5, :, 0] // U(3)
    p[5, 4:, 1] = p[5, 4:, 0] // U(3) + U(1)  # ... whose share rises by less than a ppm: delta_ppm 0
    assert int(p[:, :, 0].sum(axis=1, dtype=object).max()) < 1 << 44 and (p[:, :, 1] <= p[:, :, 0]).all()
    calls = (ProbeCall(6), ProbeCall(2), ProbeCall(6, 1 << 42), ProbeCall(6, 1, 1, True), ProbeCall(6, 1, 300_000))
    return SimpleNamespace(pairs=p, calls=calls)


def _random200():
    """70 services on 200 windows (four steps of the scan, the last of 8
    windows), a cell up to 2^30 spans, a tenth of the cells empty, a shift of
    the slow share at a drawn window for two services in three."""
    rng = np.random.default_rng(zlib.crc32(b"onset_random200"))
    S, n = 70, 200
    tot = rng.integers(0, 1 << 30, (S, n), dtype=np.uint64)
    tot[rng.random((S, n)) < 0.1] = 0
    share = np.full((S, n), 0.05) + rng.uniform(0, 0.02, (S, n))
    for s in range(S):
        if s % 3:
            share[s, rng.integers(1, n):] += rng.uniform(-0.04, 0.5)
    p = np.stack([tot, (tot.astype(np.float64) * np.clip(share, 0, 1)).astype(np.uint64)], axis=-1)
    calls = (ProbeCall(10), ProbeCall(TOP_MAX_K, 1 << 33), ProbeCall(25, 1, 1, True), ProbeCall(70, 1, 40_000))
    return SimpleNamespace(pairs=np.ascontiguousarray(p), calls=calls)


def _ties():
    """Small hand-made rows: ties of D across an empty window, equal delta_ppm
    ordered by count and then id, a quotient pair whose floors differ from the
    floor of the difference."""
    rows = [CRAFTED_PAIRS, CRAFTED_PAIRS[::-1], ((10, 1),) * 6,
            ((6, 1), (0, 0), (0, 0), (3, 1), (0, 0), (3, 1)),         # 1/6 before, 1/3 after: 333,333 - 166,666
            ((50, 0), (50, 25), (50, 25), (50, 25), (50, 25), (50, 25)),
            ((500, 0), (500, 250), (500, 250), (500, 250), (500, 250), (500, 250)),  # the same shares, ten times the spans
            ((50, 0), (50, 25), (50, 25), (50, 25), (50, 25), (50, 25)),             # ... and service 4 again
            ((0, 0),) * 6, ((7, 7), (0, 0), (0, 0), (0, 0), (0, 0), (0, 0))]          # no span; one side empty
    calls = (ProbeCall(9), ProbeCall(9, 1, 1, True), ProbeCall(3), ProbeCall(9, 200))
    return SimpleNamespace(pairs=np.array(rows, dtype=np.uint64), calls=calls)


_PROBES = {"big": _big, "random200": _random200, "ties": _ties}
PROBES = tuple(_PROBES)


@functools.lru_cache(maxsize=None)
def probe(name):
    return _PROBES[name]()


@functools.lru_cache(maxsize=None)
def want_probe(name, j):
    c = probe(name)
    return expected_probe(c.pairs, *c.calls[j].args())


def every_pairs():
    """(what, pairs [n_sel][n_cov][2], min_count, min_delta_ppm, fall, k) of every call of every workload."""
    for name in CASES:
        c = case(name)
        for j, call in enumerate(c.calls):
            p = pairs(c.ref, c.cfg, call, thresholds(c.ref, c.cfg, call))
            yield (name, j), p, call.min_count, call.min_delta_ppm, call.fall, call.k
    for name in PROBES:
        c = probe(name)
        for j, call in enumerate(c.calls):
            yield (name, j), c.pairs, call.min_count, call.min_delta_ppm, call.fall, call.k
