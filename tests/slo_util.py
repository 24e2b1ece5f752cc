"""sa_window_slo: the numpy restatement the GPU tests compare with, built on
tests/latency_util.py, and the workloads both the GPU tests and the host tests
(tests/test_window_slo_host.py, which holds spanagg.sketch's plain-Python
rules against it) run.

  expected   per output t, width w and selected service i: total = the spans of
             windows t - w + 1 .. t, slow = those in bins above the bin of the
             service's threshold; bit w of burning[t][i] = total >= max(
             min_count, 1) and slow * 10^6 > limit_ppm[w] * total (strictly);
             alert_outputs[i] = the outputs whose bits are all set

The `wrong` switch builds the references that make a known mistake: "ge_bin"
(the threshold's own bin counted slow), "nonstrict" (>= in the burn rule),
"no_min_count" (the min_count rule dropped), "any_width" (an alert when any
width burns).  The host tests show that the workloads tell each from the right
one.

A case is its configuration, the (ring base, batch) steps that fill the ring,
the per-window histograms after them (computed once, shared and never
changed) and the calls made against it.
"""
import dataclasses
import functools
import zlib
from types import SimpleNamespace

import numpy as np

import latency_util as lu
from geometry_util import config_of, make_batch, ring_start
from spanagg import Config, SpanBatch, pack_meta
from spanagg._lib import OPT_WINDOW_LATENCY

U = np.uint64
WRONG = ("ge_bin", "nonstrict", "no_min_count", "any_width")
BIN_LO = np.concatenate([[U(0)], lu.BIN_HI[:-1] + U(1)]).astype(np.uint64)
FIELDS = ("services", "widths", "limit_ppm", "threshold_ns", "threshold_bin", "effective_ns", "total", "slow", "burning",
          "alert_outputs")


@dataclasses.dataclass(frozen=True)
class Call:
    first: int
    last: int
    widths: tuple
    limit_ppm: tuple
    thresholds: tuple           # one a selected service (every service when services is None)
    services: tuple = None
    min_count: int = 1

    def args(self):
        """As Engine.window_slo takes them."""
        return (self.first, self.last, self.widths, self.limit_ppm, self.thresholds, self.services, self.min_count)


def expected(ref, cfg, call, wrong=None):
    """What window_slo(*call.args()) must return, as a namespace of FIELDS
    (and first, last, min_count)."""
    sel = np.arange(cfg.n_services) if call.services is None else np.asarray(call.services, dtype=np.int64)
    thr = np.asarray(call.thresholds, dtype=np.uint64)
    assert thr.shape == sel.shape
    tb = lu.bins_of(thr)
    mw, n_out, W = max(call.widths), call.last - call.first + 1, len(call.widths)
    h = lu.ring_hists(ref, cfg, call.first - mw + 1, call.last)[:, sel]  # [n_cov][n_sel][256]
    bins = np.arange(lu.BINS)
    above = bins[None, :] >= tb[:, None] if wrong == "ge_bin" else bins[None, :] > tb[:, None]
    tot = h.sum(axis=-1, dtype=np.uint64)
    slo = np.where(above[None], h, U(0)).sum(axis=-1, dtype=np.uint64)
    total = np.zeros((n_out, W, len(sel)), np.uint64)
    slow = np.zeros_like(total)
    for w, width in enumerate(call.widths):  # (row o of a slide covers covered windows o .. o + width - 1)
        total[:, w] = lu.sliding(tot, width)[mw - width:]
        slow[:, w] = lu.sliding(slo, width)[mw - width:]
    mc = U(1 if wrong == "no_min_count" else max(call.min_count, 1))
    lhs, rhs = slow * U(1_000_000), np.asarray(call.limit_ppm, dtype=np.uint64)[None, :, None] * total
    burns = (total >= mc) & ((lhs >= rhs) if wrong == "nonstrict" else (lhs > rhs))
    burning = np.zeros((n_out, len(sel)), np.uint8)
    for w in range(W):
        burning |= burns[:, w].astype(np.uint8) << np.uint8(w)
    alert = burns.any(axis=1) if wrong == "any_width" else burns.all(axis=1)
    return SimpleNamespace(
        first=call.first, last=call.last, min_count=max(call.min_count, 1), services=sel.astype(np.uint32),
        widths=np.asarray(call.widths, np.uint32), limit_ppm=np.asarray(call.limit_ppm, np.uint32), threshold_ns=thr,
        threshold_bin=tb.astype(np.uint8), effective_ns=lu.BIN_HI[tb], total=total, slow=slow, burning=burning,
        alert_outputs=alert.sum(axis=0).astype(np.uint32))


def assert_slo(res, want, what=""):
    assert (res.first, res.last, res.min_count) == (want.first, want.last, want.min_count), what
    for f in FIELDS:
        a, b = getattr(res, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), (f, what)


def same(a, b, what=""):
    """Two results field by field."""
    assert_slo(a, b, what)


def spans(cfg, window, services, durations) -> SpanBatch:
    """One span a (service, duration) pair, all ending in `window`."""
    n = len(durations)
    end = np.full(n, window * cfg.window_ns + 5, dtype=np.uint64)
    k = np.arange(1, n + 1, dtype=np.uint64)
    return SpanBatch(k, end - np.asarray(durations, dtype=np.uint64), end, k, k,
                     pack_meta(np.asarray(services), np.zeros(n), np.zeros(n)))


def _cfg(S, W) -> Config:
    return Config(n_services=S, n_windows=W, hll_p=10, key_capacity=1000, options=OPT_WINDOW_LATENCY)


def _case(cfg, steps, calls, **more):
    return SimpleNamespace(cfg=cfg, steps=steps, ref=lu.window_hists(cfg, steps), calls=calls, **more)


# thresholds the drawn workloads pick from: both ends, the linear bins, bins'
# upper bounds (exact) and values inside a bin (a lower bound), the open last bin
THRESHOLDS = (0, 127, 128, 1_000, 99_999, int(lu.BIN_HI[100]), 1_000_000, int(lu.BIN_HI[141]), 50_000_000,
              1_000_000_000, 1 << 62, (1 << 64) - 1)


def _thresholds(rng, n):
    return tuple(int(THRESHOLDS[j]) for j in rng.integers(0, len(THRESHOLDS), n))


def _every_bin():
    """256 services with one span in each of the 256 bins (at the bins' lower
    bounds) of the ring's second window; service s's threshold is the lower
    bound of bin s: slow == 255 - s of total == 256."""
    cfg = _cfg(256, 2)
    w0 = ring_start(cfg)
    svc, b = np.divmod(np.arange(256 * 256), 256)
    thr = tuple(int(v) for v in BIN_LO)
    calls = [Call(w0 + 1, w0 + 1, (1, 2), (0, 500_000), thr), Call(w0, w0 + 1, (1,), (990_000,), thr)]
    return _case(cfg, [(w0, spans(cfg, w0 + 1, svc, BIN_LO[b]))], calls, w0=w0)


def _services(S):
    """Every service of S on 8 windows, widths (1, 3, 8), first == last."""
    cfg = _cfg(S, 8)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"slo_svc") + S)
    batch = make_batch(rng, 100_000, cfg, 500, w0=w0)
    calls = [Call(w0 + 7, w0 + 7, (1, 3, 8), (500_000, 200_000, 50_000), _thresholds(rng, S), None, 40)]
    return _case(cfg, [(w0, batch)], calls, w0=w0)


def _moved():
    """ring_1024_noerr's 32 windows (one service), moved by 13: the resident
    windows wrap the slots.  The windows both batches cover hold about 3,700
    spans, the others about 1,850: min_count 3,000 parts them at width 1."""
    cfg = config_of("ring_1024_noerr")
    cfg = dataclasses.replace(cfg, options=cfg.options | OPT_WINDOW_LATENCY)
    rng = np.random.default_rng(zlib.crc32(b"slo_moved"))
    w0 = ring_start(cfg)
    base = w0 + 13
    steps = [(w0, make_batch(rng, 60_000, cfg, 700, w0=w0)), (base, make_batch(rng, 60_000, cfg, 700, w0=base))]
    calls = [Call(base + 4, base + 31, (1, 2, 5), (100_000, 300_000, 400_000), (1_000_000,), None, 3_000),
             Call(base + 31, base + 31, (31, 32), (350_000, 1_000), (int(lu.BIN_HI[120]),))]
    return _case(cfg, steps, calls, base=base)


def _long():
    """A 128-window ring, 100 outputs, widths (29, 1): 128 covered windows are
    two 64-window chunks of the scan; 99 outputs from one window later, 127 covered."""
    cfg = _cfg(3, 128)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"slo_long"))
    thr = (250_000, int(lu.BIN_HI[150]), 0)
    calls = [Call(w0 + 28, w0 + 127, (29, 1), (300_000, 300_000), thr, None, 200),
             Call(w0 + 29, w0 + 127, (29, 1), (300_000, 300_000), thr, None, 200)]
    return _case(cfg, [(w0, make_batch(rng, 100_000, cfg, 500, w0=w0))], calls, w0=w0)


def _selection():
    """An unsorted selection of 12 services, a threshold each."""
    cfg = _cfg(12, 4)
    w0 = ring_start(cfg)
    rng = np.random.default_rng(zlib.crc32(b"slo_sel"))
    sel, thr = (7, 2, 11, 0), (1_000_000, 127, (1 << 64) - 1, 20_000_000)
    calls = [Call(w0 + 1, w0 + 3, (2, 1), (250_000, 250_000), thr, sel, 100),
             Call(w0 + 1, w0 + 3, (2, 1, 2, 1), (250_000, 250_000, 0, 1_000_000), thr, sel, 0)]
    return _case(cfg, [(w0, make_batch(rng, 50_000, cfg, 500, w0=w0))], calls, w0=w0)


CRAFTED_THRESHOLD = int(lu.BIN_HI[100])  # a bin's upper bound: exact
CRAFTED_FAST, CRAFTED_SLOW = int(lu.BIN_HI[100]), int(lu.BIN_HI[100]) + 1  # the threshold's own bin; the next


def _crafted():
    """One service on four windows.  Step 0: window w0 + 1 takes 1,000 spans,
    10 of them above the threshold.  Step 1: an 11th slow span there.  Step 2:
    window w0 + 3 takes 100 spans, 50 of them slow; w0 and w0 + 2 stay empty.
    calls[j]: (the steps fed before it, the call, the burning bits of every
    output, alert_outputs) -- written by hand from the rule."""
    cfg = _cfg(1, 4)
    w0 = ring_start(cfg)
    d = lambda fast, slow: [CRAFTED_FAST] * fast + [CRAFTED_SLOW] * slow
    steps = [(w0, spans(cfg, w0 + 1, np.zeros(1000), d(990, 10))), (w0, spans(cfg, w0 + 1, np.zeros(1), d(0, 1))),
             (w0, spans(cfg, w0 + 3, np.zeros(100), d(50, 50)))]
    t, thr = w0 + 1, (CRAFTED_THRESHOLD,)
    one = lambda limit, mc=1, th=thr: Call(t, t, (1,), (limit,), th, None, mc)
    calls = [
        (1, one(10_000), [0], 0),            # 10 * 10^6 == 10,000 * 1,000: equal products do not burn
        (1, one(9_999), [1], 1),
        (1, one(9_999, 1_000), [1], 1),      # total == min_count
        (1, one(9_999, 1_001), [0], 0),
        (1, one(0, 1, (CRAFTED_SLOW,)), [0], 0),   # slow == 0: 0 > 0 is false
        (1, one(1_000_000, 1, (0,)), [0], 0),      # every span slow: 10^6 * total is not above itself
        (1, one(999_999, 1, (0,)), [1], 1),
        (2, one(10_000), [1], 1),            # 11 * 10^6 > 10,000 * 1,001
        # outputs w0 + 1 .. w0 + 3: (1,001, 11) both widths; nothing at width 1, (1,001, 11) at width 2; (100, 50) both
        (3, Call(w0 + 1, w0 + 3, (1, 2), (10_000, 10_000), thr), [3, 2, 3], 2),
        (3, Call(w0 + 1, w0 + 3, (1, 2), (10_000, 600_000), thr), [1, 0, 1], 0),
        (3, Call(w0 + 1, w0 + 3, (2, 1), (10_000, 400_000), thr), [1, 1, 3], 1),
    ]
    refs = [lu.window_hists(cfg, steps[:n]) for n in range(len(steps) + 1)]
    return SimpleNamespace(cfg=cfg, steps=steps, refs=refs, calls=calls, w0=w0)


_BUILD = {"every_bin": _every_bin, "moved": _moved, "long": _long, "selection": _selection,
          **{f"services{S}": functools.partial(_services, S) for S in (1, 64, 129, 1000)}}
CASES = tuple(_BUILD)


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILD[name]()


@functools.lru_cache(maxsize=None)
def crafted():
    return _crafted()


@functools.lru_cache(maxsize=None)
def want(name, j):
    """expected() of call j of case `name`, computed once."""
    c = case(name)
    return expected(c.ref, c.cfg, c.calls[j])


def every_call():
    """(what, ref, cfg, call) of every call of every workload, the crafted ones included."""
    for name in CASES:
        c = case(name)
        for j, call in enumerate(c.calls):
            yield (name, j), c.ref, c.cfg, call
    c = crafted()
    for j, (n, call, _, _) in enumerate(c.calls):
        yield ("crafted", j), c.refs[n], c.cfg, call
