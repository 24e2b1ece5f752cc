"""sa_window_latency, the parts that need no GPU: the two host helpers against
the plain-Python rules of spanagg.sketch, the numpy reference of
tests/latency_util.py against those rules, and -- on the reference alone --
that the workloads of tests/test_gpu_window_latency.py can tell a right engine
from one that makes the mistakes they are there for."""
import ctypes as C
import functools
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import latency_util as lu
from geometry_util import config_of, make_batch, ring_start
from spanagg import LAT_BINS, LAT_MAX_Q, SpanBatch, _lib, pack_meta, sketch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def latency_bin(d_ns: int) -> int:
    """sa_latency_bin through ctypes."""
    return int(_lib.load().sa_latency_bin(int(d_ns)))


def latency_bin_bounds(b: int):
    """sa_latency_bin_bounds through ctypes: (lo, hi)."""
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    assert _lib.load().sa_latency_bin_bounds(int(b), C.byref(lo), C.byref(hi)) == _lib.SA_OK, b
    return int(lo.value), int(hi.value)


def test_constants_and_option_bit():
    assert (LAT_BINS, LAT_MAX_Q, _lib.SA_LAT_HIST, sketch.LAT_BINS) == (256, 8, 1, 256)
    assert _lib.OPT_WINDOW_LATENCY == 1 << 10
    text = open(os.path.join(ROOT, "include", "spanagg.h")).read()
    for line in ("#define SA_OPT_WINDOW_LATENCY (1u << 10)", "#define SA_OPT_ALL           0x7FFu",
                 "#define SA_LAT_BINS  256u", "#define SA_LAT_MAX_Q 8u", "#define SA_ABI_VERSION 4"):
        assert line in text, line
    assert C.sizeof(_lib.sa_latency_result) == 80


def test_bin_of_every_edge_matches_the_rule():
    """Every bin's lo - 1, lo, hi, hi + 1, and the two ends of the range."""
    for b in range(LAT_BINS):
        lo, hi = latency_bin_bounds(b)
        assert (lo, hi) == sketch.latency_bin_bounds(b), b
        for d in (lo - 1, lo, hi, hi + 1):
            if 0 <= d <= M64:
                assert latency_bin(d) == sketch.latency_bin(d), d
        assert latency_bin(lo) == latency_bin(hi) == b
        if b:
            assert latency_bin(lo - 1) == b - 1
        if b < LAT_BINS - 1:
            assert latency_bin(hi + 1) == b + 1
    assert latency_bin(0) == 0 and latency_bin(M64) == 255
    assert latency_bin_bounds(255) == (15 << 37, M64)
    assert latency_bin_bounds(16) == (2048, 2048 + 255)


def test_bounds_tile_the_range_and_widths():
    nxt = 0
    for b in range(LAT_BINS):
        lo, hi = latency_bin_bounds(b)
        assert lo == nxt and hi >= lo, b
        if b < 16:
            assert hi - lo == 127
        elif b < LAT_BINS - 1:
            assert (hi - lo + 1) * 8 <= lo, b  # at most 12.5 % of its lower bound
        nxt = hi + 1
    assert nxt == 1 << 64


def test_bin_is_monotone():
    rng = np.random.default_rng(3)
    d = np.unique(np.concatenate([np.exp(rng.uniform(0, np.log(2.0 ** 63.9), 4000)).astype(np.uint64),
                                  np.array([0, 1, 127, 128, 2047, 2048, M64], dtype=np.uint64)]))
    bins = [latency_bin(int(x)) for x in d]
    assert bins == sorted(bins) and bins[0] == 0 and bins[-1] == 255
    assert np.array_equal(lu.bins_of(d), np.array(bins))
    assert [sketch.latency_bin(int(x)) for x in d] == bins


def test_bounds_reject_a_bin_past_the_last():
    lib = _lib.load()
    lo, hi = C.c_uint64(7), C.c_uint64(7)
    assert lib.sa_latency_bin_bounds(256, C.byref(lo), C.byref(hi)) == _lib.SA_EINVAL
    assert lib.sa_latency_bin_bounds(2 ** 32 - 1, C.byref(lo), C.byref(hi)) == _lib.SA_EINVAL
    assert lib.sa_latency_bin_bounds(3, None, C.byref(hi)) == _lib.SA_EINVAL
    assert (lo.value, hi.value) == (7, 7)
    with pytest.raises(ValueError):
        sketch.latency_bin_bounds(256)


def test_vectorised_bins_match_the_rule_at_every_edge():
    edges = sorted({d for b in range(LAT_BINS) for lo, hi in [sketch.latency_bin_bounds(b)]
                    for d in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1) if 0 <= d <= M64})
    got = lu.bins_of(np.array(edges, dtype=np.uint64))
    assert got.tolist() == [sketch.latency_bin(d) for d in edges]
    assert lu.BIN_HI[255] == M64 and lu.BIN_HI[0] == 127


def test_vectorised_quantiles_match_the_rule():
    rng = np.random.default_rng(11)
    rows = np.zeros((40, LAT_BINS), np.uint64)
    for r in range(1, 40):  # row 0 stays empty
        where = rng.integers(0, LAT_BINS, rng.integers(1, 30))
        rows[r, where] = rng.integers(1, 10 ** rng.integers(1, 7), len(where))
    ppm = [1, 333_333, 333_334, 500_000, 950_000, 990_000, 999_999, 1_000_000]
    count, q_bin, q_ns = lu.quantile_bins(rows, ppm)
    for r in range(40):
        assert int(count[r]) == int(rows[r].sum())
        want = [sketch.latency_quantile_bin(rows[r], q) for q in ppm]
        assert q_bin[r].tolist() == want, r
        assert q_ns[r].tolist() == [sketch.latency_bin_bounds(b)[1] if count[r] else 0 for b in want]
    assert not q_bin[0].any() and not q_ns[0].any()


def _crafted(a, b, c):
    row = np.zeros(LAT_BINS, np.uint64)
    for x in (a, b, c):
        row[x] += 1
    return row


def test_rank_edges_on_crafted_rows():
    """Three spans in bins a < b < c: 333,333 ppm is rank ceil(0.999999) = 1,
    333,334 ppm rank ceil(1.000002) = 2; 1 ppm the first span, 10^6 the last."""
    a, b, c = 3, 77, 255
    row = _crafted(a, b, c)
    ppm = [333_333, 333_334, 1, 1_000_000, 666_666, 666_667]
    assert [sketch.latency_quantile_bin(row, q) for q in ppm] == [a, b, a, c, b, c]
    assert lu.quantile_bins(row[None], ppm)[1][0].tolist() == [a, b, a, c, b, c]
    assert lu.quantile_bins(row[None], ppm, wrong="floor_rank")[1][0].tolist() == [a, a, a, c, a, b]
    one = np.zeros(LAT_BINS, np.uint64)
    one[200] = 1
    assert [sketch.latency_quantile_bin(one, q) for q in (1, 500_000, 1_000_000)] == [200, 200, 200]
    empty = np.zeros(LAT_BINS, np.uint64)
    assert [sketch.latency_quantile_bin(empty, q) for q in (1, 1_000_000)] == [0, 0]
    count, q_bin, q_ns = lu.quantile_bins(np.stack([one, empty]), [1, 1_000_000])
    assert count.tolist() == [1, 0] and q_bin.tolist() == [[200, 200], [0, 0]]
    assert q_ns.tolist() == [[int(lu.BIN_HI[200])] * 2, [0, 0]]


@functools.lru_cache(maxsize=1)
def _ring_512():
    cfg = config_of("ring_512")
    rng = np.random.default_rng(zlib.crc32(b"window_latency_host"))
    w0 = ring_start(cfg)
    return cfg, w0, make_batch(rng, 200_000, cfg, 500, w0=w0)


def test_workload_reaches_the_ends_and_the_middle():
    """make_batch's durations: log-uniform from 1 ns to 6e10 ns (4 x the
    15,000 ms bound), 2 % zero, 2 % end < start, one 2^62 per series."""
    cfg, w0, batch = _ring_512()
    ref = lu.window_hists(cfg, [(w0, batch)])
    total = lu.ring_hists(ref, cfg, w0, w0 + cfg.n_windows - 1).sum(axis=(0, 1))
    assert total[0] > 0 and total[255] > 0
    assert int((total[1:255] > 0).sum()) >= 100
    ok = ((batch.meta & 0xFFFF) < cfg.n_services) & (batch.end_ns // np.uint64(cfg.window_ns) >= w0) & \
         (batch.end_ns // np.uint64(cfg.window_ns) < w0 + cfg.n_windows)
    assert int(total.sum()) == int(ok.sum()) < len(batch)  # (some spans are out of the ring or of the services)
    assert set(ref) <= set(range(w0, w0 + cfg.n_windows))


@pytest.mark.parametrize("wrong", ["by_start", "invalid_services", "no_clamp"])
def test_workload_tells_a_wrong_histogram(wrong):
    cfg, w0, batch = _ring_512()
    last = w0 + cfg.n_windows - 1
    right = lu.ring_hists(lu.window_hists(cfg, [(w0, batch)]), cfg, w0, last)
    bad = lu.ring_hists(lu.window_hists(cfg, [(w0, batch)], wrong=wrong), cfg, w0, last)
    assert not np.array_equal(right, bad)


def test_crafted_workload_tells_a_rank_rounded_down():
    """The crafted spans of the GPU test: 333,334 ppm of three spans is rank 2
    (ceil 1.000002), 666,667 ppm rank 3; rounded down they are ranks 1 and 2."""
    cfg, w0, _ = _ring_512()
    ref = lu.window_hists(cfg, [(w0, lu.crafted_batch(cfg, w0 + 1))])
    h = lu.ring_hists(ref, cfg, w0 + 1, w0 + 1)[0]
    assert h[0].nonzero()[0].tolist() == list(lu.CRAFTED_BINS) and h[1].nonzero()[0].tolist() == [200]
    count, q_bin, q_ns = lu.quantile_bins(h, lu.CRAFTED_PPM)
    assert count.tolist() == [3, 1] and q_bin[0].tolist() == list(lu.CRAFTED_WANT) and q_bin[1].tolist() == [200] * 6
    assert q_ns[0, 3] == M64 and q_ns[0, 0] == 3 * 128 + 127
    wrong = lu.quantile_bins(h, lu.CRAFTED_PPM, wrong="floor_rank")[1]
    assert not np.array_equal(q_bin, wrong)


def test_retired_windows_leave_the_reference():
    """A later base drops the windows below it, and a span whose end lay
    outside the ring at its own step stays out whatever the ring does later."""
    cfg, w0, batch = _ring_512()
    W, a = cfg.n_windows, cfg.n_windows // 2
    nothing = SpanBatch(*[c[:0] for c in batch.columns()])
    early = lu.window_hists(cfg, [(w0, batch), (w0 + a, nothing)])
    late = lu.window_hists(cfg, [(w0 + a, batch)])
    assert set(early) == set(range(w0 + a, w0 + W))
    assert w0 + W in late  # (make_batch puts ~0.5 % of the ends in the window after its ring)
    for w in range(w0 + a, w0 + W):
        assert np.array_equal(late[w], early[w]), w


def test_sliding_sums_equal_direct_sums():
    rng = np.random.default_rng(5)
    h = rng.integers(0, 1000, (9, 3, LAT_BINS)).astype(np.uint64)
    for width in (1, 2, 8, 9):
        s = lu.sliding(h, width)
        assert s.shape[0] == 9 - width + 1
        for o in range(s.shape[0]):
            assert np.array_equal(s[o], h[o:o + width].sum(axis=0)), (width, o)


def test_create_refuses_an_oversized_ring_before_any_device():
    """n_windows * n_services > 2^18 with the option: SA_EINVAL from the
    config check, with or without a GPU; the same shapes without the option
    and the option at the bound pass that check."""
    from spanagg import Config, Engine
    for W, S in ((4096, 65), (8, 32769)):
        with pytest.raises(_lib.SpanAggError) as x:
            Engine(Config(n_services=S, n_windows=W, hll_p=4, options=_lib.OPT_WINDOW_LATENCY))
        assert x.value.code == _lib.SA_EINVAL, (W, S)
    lib = _lib.load()
    for W, S, opt in ((4096, 65, 0), (4096, 64, _lib.OPT_WINDOW_LATENCY)):
        c, keep = Config(n_services=S, n_windows=W, hll_p=4, options=opt, device=10 ** 6).to_c()
        h = C.c_void_p()
        assert lib.sa_create(C.byref(c), C.byref(h)) == _lib.SA_EDEVICE and not h  # (no such device: past the checks)


def test_python_wrappers_map_quantiles_to_ppm():
    assert lu.ppm_of((0.5, 0.95, 0.99, 0.999999, 1.0, 1e-6)) == [500_000, 950_000, 990_000, 999_999, 1_000_000, 1]
    m = pack_meta([1], [0], [0])
    assert int(m[0]) & 0xFFFF == 1


def test_host_helpers_under_sanitizers(tmp_path):
    """The bin rule as a stand-alone host program with its own main
    (tools/latency_bins_check.cpp), built with -fsanitize=address,undefined
    and run: the sweep of every bin edge, clean."""
    cxx = shutil.which("c++") or shutil.which("g++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "latency_bins_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "opentelemetry-demo_amd", "csrc"),
                    os.path.join(ROOT, "tools", "latency_bins_check.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"))
    assert run.returncode == 0 and "latency bins ok" in run.stdout, run.stderr
