"""Latency histograms over the window ring (SA_OPT_WINDOW_LATENCY): the numpy
restatement the GPU tests compare with, held against the plain-Python rules of
spanagg.sketch by tests/test_window_latency_host.py.

  bins_of        the bin of every duration of an array (integer arithmetic only)
  window_hists   per resident window [n_services][256] counts after a list of
                 (ring base, batch) steps: a span counts when its service is
                 valid and its end lies inside the ring as it stood at its
                 step; windows retired since are dropped
  sliding        every trailing span's sums from a cumulative sum
  quantile_bins  rank r = max(1, ceil(count * ppm / 10^6)), the first bin whose
                 cumulative count reaches it

The `wrong` switches of window_hists and quantile_bins build the references
that make a known mistake; the host tests show that the workloads tell them
from the right one.
"""
import numpy as np

from spanagg import sketch

BINS = 256
BIN_HI = np.array([sketch.latency_bin_bounds(b)[1] for b in range(BINS)], dtype=np.uint64)
U = np.uint64


def bins_of(d) -> np.ndarray:
    """sketch.latency_bin of every element of d (u64)."""
    q = np.asarray(d, dtype=np.uint64) >> U(7)
    e, t = np.zeros(q.shape, np.int64), q.copy()
    for s in (32, 16, 8, 4, 2, 1):  # floor(log2 q) by halving
        m = t >= (U(1) << U(s))
        e += np.where(m, s, 0)
        t = np.where(m, t >> U(s), t)
    sh = np.maximum(e - 3, 0)
    log = np.minimum(BINS - 1, (sh << 3) + (q >> sh.astype(np.uint64)).astype(np.int64))
    return np.where(q < 16, q.astype(np.int64), log)


def durations(batch, clamp=True) -> np.ndarray:
    """end > start ? end - start : 0 (clamp=False: the wrapped difference)."""
    d = batch.end_ns - batch.start_ns
    return np.where(batch.end_ns > batch.start_ns, d, U(0)) if clamp else d


def window_hists(cfg, steps, wrong=None) -> dict:
    """{window: [n_services][256] u64} after the steps; a window that is
    resident and absent is all zero.  wrong: None, "by_start" (the window of
    the start time), "invalid_services" (a service past the last counts as
    the last), "no_clamp" (end < start not taken as 0)."""
    S, W, wns = cfg.n_services, cfg.n_windows, U(cfg.window_ns)
    ref = {}
    for base, b in steps:
        for w in [w for w in ref if w < base]:
            del ref[w]
        svc = (b.meta & np.uint32(0xFFFF)).astype(np.int64)
        win = (b.start_ns if wrong == "by_start" else b.end_ns) // wns
        ok = (win >= U(base)) & (win < U(base + W))
        if wrong == "invalid_services":
            svc = np.minimum(svc, S - 1)
        else:
            ok &= svc < S
        bins = bins_of(durations(b, clamp=wrong != "no_clamp"))
        for w in np.unique(win[ok]):
            m = ok & (win == w)
            h = ref.setdefault(int(w), np.zeros((S, BINS), np.uint64))
            np.add.at(h, (svc[m], bins[m]), U(1))
    return ref


def ring_hists(ref, cfg, first, last) -> np.ndarray:
    """[last - first + 1][n_services][256] of the windows first..last."""
    zero = np.zeros((cfg.n_services, BINS), np.uint64)
    return np.stack([ref.get(w, zero) for w in range(first, last + 1)])


def sliding(h, width) -> np.ndarray:
    """h [n_in][...] -> [n_in - width + 1][...]: row o = h[o .. o + width - 1] summed."""
    c = np.concatenate([np.zeros((1,) + h.shape[1:], np.uint64), np.cumsum(h, axis=0, dtype=np.uint64)])
    return c[width:] - c[:-width]


def quantile_bins(hist, q_ppm, wrong=None):
    """hist [..., 256] -> (count [...], q_bin [..., n_q] u8, q_ns [..., n_q] u64).
    wrong="floor_rank": the rank rounded down."""
    c = np.cumsum(hist, axis=-1, dtype=np.uint64)
    count = c[..., -1]
    out = np.zeros(count.shape + (len(q_ppm),), np.uint8)
    for i, ppm in enumerate(q_ppm):
        prod = count * U(int(ppm))
        r = prod // U(1_000_000) if wrong == "floor_rank" else (prod + U(999_999)) // U(1_000_000)
        r = np.maximum(r, U(1))
        out[..., i] = np.where(count > 0, (c >= r[..., None]).argmax(axis=-1), 0)
    q_ns = np.where(count[..., None] > 0, BIN_HI[out], U(0))
    return count, out, q_ns


CRAFTED_BINS = (3, 77, 255)  # a < b < c: the linear bins, the log bins, the open last bin
CRAFTED_PPM = (333_333, 333_334, 1, 1_000_000, 666_666, 666_667)
CRAFTED_WANT = (3, 77, 3, 255, 77, 255)  # ranks 1, 2, 1, 3, 2, 3


def crafted_batch(cfg, window) -> "SpanBatch":
    """The rank edges as spans of `window`: service 0 has one span in each of
    CRAFTED_BINS (at the bins' lower bounds), service 1 one span at the upper
    bound of bin 200, every other service none."""
    from spanagg import SpanBatch, pack_meta
    d = [sketch.latency_bin_bounds(b)[0] for b in CRAFTED_BINS] + [sketch.latency_bin_bounds(200)[1]]
    end = np.full(4, window * cfg.window_ns + 5, dtype=np.uint64)
    start = end - np.array(d, dtype=np.uint64)
    k = np.arange(1, 5, dtype=np.uint64)
    return SpanBatch(k, start, end, k, k, pack_meta([0, 0, 0, 1], [0] * 4, [0] * 4))


def ppm_of(quantiles):
    return [int(round(float(q) * 1e6)) for q in quantiles]


def expected(ref, cfg, first, last, width, services, quantiles):
    """What window_latency_series(first, last, width, services, quantiles,
    hist=True) must return: (count, q_bin, q_ns, hist)."""
    h = sliding(ring_hists(ref, cfg, first - width + 1, last), width)
    if services is not None:
        h = h[:, np.asarray(services, dtype=np.int64)]
    return quantile_bins(h, ppm_of(quantiles)) + (h,)


def assert_latency(res, want, what=""):
    count, q_bin, q_ns, hist = want
    assert np.array_equal(res.count, count), ("count", what)
    if res.hist is not None:
        assert np.array_equal(res.hist, hist), ("hist", what)
    assert np.array_equal(res.q_bin, q_bin), ("q_bin", what)
    assert np.array_equal(res.q_ns, q_ns), ("q_ns", what)
