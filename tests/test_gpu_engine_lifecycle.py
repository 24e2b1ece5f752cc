"""Engine lifetime and ordering on every ingest path: 8 cycles of create, host
ingest, device ingest on a second stream, flush, window read, stats, destroy,
at the smallest config that reaches each of the seven paths (sa_path.h
decide_path; the configs are test_path_decision.py's).  The shapes are tiny on
purpose: the test is about what an engine owns and in which order it waits,
not throughput.

Checks per path:
- `small_table` of sa_stats agrees with the path (1: Small, ExpoSmall);
- cycle 1's flush equals the CPU oracle: parity_util.assert_red_equal for the
  explicit-bucket paths; exponential engines flush through flush_exp, whose
  result assert_red_equal cannot take, so they are held to pyoracle's
  expo_aggregate the way test_gpu_expo.py does (counts, scale, offset, buckets,
  min, max exact, sums within 1e-9 relative);
- free device memory after cycle 8's destroy has not dropped below the value
  after cycle 2's by more than MARGIN (torch.cuda.mem_get_info after a device
  synchronise; cycles 1-2 absorb what the runtime and torch keep for good).

MARGIN.  The parent commit (one hand-kept free list in sa_destroy, nothing
left out) ran this file on the same MI355X: its drift between cycle 2 and
cycle 8 was 0 bytes on all seven paths (free memory read the same after every
one of the eight destroys), and so is this tree's.  Twice the parent's largest
drift is 0, so MARGIN is 0: any drop fails.  What the guard can see is set by
the runtime, measured on the same machine with raw hipMalloc calls: it hands
out small allocations from chunks of 2 MiB and mem_get_info moves only when
it takes or returns a chunk (1 x 64 B, 6 x 64 B and 6 x 64 KiB each moved it
by 2 MiB; 6 x 512 KiB by 4 MiB).  A buffer leaked once per engine is therefore
certain to show when six cycles of it pass 2 MiB (>= 350 KiB per engine: every
table, slab set, record set, staging slot and flush buffer of these configs
except the 2^11-slot engines' 16 KiB key table and error counts), and shows
by luck below that: the guard is blind to a leak of the 64-byte stats /
scratch / seed buffers, the bin table (2 KiB), hll_filt (8 KiB), the pool
ring, and of events and streams, which hold no device memory it can see.
"""
import functools

import numpy as np
import pytest

import pyoracle
from parity_util import SUM_RTOL, assert_red_equal
from spanagg import Config, Engine
from spanagg._lib import OPT_ATOMIC_TABLE, OPT_DENSE_IDS, OPT_EXPO_HBM
from spanagg.synth import generate_c2

pytestmark = pytest.mark.gpu

MARGIN = 0  # bytes; see the module docstring
CYCLES = 8
N = 4096  # spans per ingest call

# path -> (config fields, small_table)
PATHS = {
    "small": (dict(key_capacity=1000), 1),
    "expo_small": (dict(key_capacity=1000, exp_max_size=160), 1),
    "expo_hbm": (dict(key_capacity=1000, exp_max_size=160, options=OPT_EXPO_HBM), 0),
    "partitioned": (dict(key_capacity=200_000), 0),
    "binned": (dict(key_capacity=300_000), 0),
    "dense": (dict(key_capacity=1000, options=OPT_DENSE_IDS), 0),
    "atomic": (dict(key_capacity=300_000, options=OPT_ATOMIC_TABLE), 0),
}


@functools.lru_cache(maxsize=None)
def _workload():
    """5 N spans: host [0, N), device [N, 2N), the small path's graph of
    three [2N, 5N); the oracles of the first 2 N and of all of them."""
    wl = generate_c2(5 * N, seed=23)
    two, five = wl.batch.slice(0, 2 * N), wl.batch
    ora = {}
    for name, b in (("two", two), ("five", five)):
        o = pyoracle.Oracle(n_services=wl.n_services)
        o.ingest(b)
        ora[name] = (b, o)
    return wl, ora


def _assert_expo_equal(res, batch, max_size):
    ora = pyoracle.expo_aggregate(batch, max_size, False)
    assert [int(k) for k in res.key_hash] == sorted(ora)
    for i, k in enumerate(int(k) for k in res.key_hash):
        o = ora[k]
        assert (int(res.count[i]), int(res.zero_count[i])) == (o["count"], o["zero_count"]), k
        assert (int(res.scale[i]), int(res.offset[i])) == (o["scale"], o["offset"]), k
        assert [int(x) for x in res.buckets[i]] == [int(x) for x in o["counts"]], k
        assert res.min[i] == o["min"] and res.max[i] == o["max"], k
        assert abs(res.sum[i] - o["sum"]) <= SUM_RTOL * max(abs(o["sum"]), 1e-300), k


def _free(dev):
    import torch
    torch.cuda.synchronize(dev)
    return torch.cuda.mem_get_info(dev)[0]


@pytest.mark.parametrize("path", list(PATHS))
def test_cycles_own_and_release_everything(path):
    import torch
    dev = torch.device("cuda", 0)
    fields, small_table = PATHS[path]
    wl, ora = _workload()
    batch, o = ora["five" if path == "small" else "two"]
    cfg = Config(n_services=wl.n_services, n_windows=16, device=0, **fields)
    side = torch.cuda.Stream(dev)
    free = []
    for cycle in range(1, CYCLES + 1):
        with Engine(cfg) as e:
            e.window_advance(wl.first_window)
            keys = batch.key_hash
            if path == "dense":  # indices for the device batch, bound first
                keys, new_i, new_h = e.ids.encode(batch.key_hash)
                e.bind_ids(new_i, new_h)
                keys = np.ascontiguousarray(keys, dtype=np.uint64)
            cols = [torch.from_numpy(c.view(np.int64) if c.dtype == np.uint64 else c.view(np.int32)).to(dev)
                    for c in (keys,) + tuple(batch.columns()[1:])]
            side.wait_stream(torch.cuda.current_stream(dev))  # (the columns' copies)
            e.ingest(batch.slice(0, N))
            e.ingest_device(*[c[N:2 * N] for c in cols], stream=side.cuda_stream)
            if path == "small":
                e.ingest_device_many([tuple(c[a:a + N] for c in cols) for a in (2 * N, 3 * N, 4 * N)],
                                     stream=side.cuda_stream)
            res = e.flush_exp() if cfg.exp_max_size else e.flush()
            wid = o.window_ids()[0]
            sk = e.window_read(wid)
            st = e.stats()
            assert st["small_table"] == small_table
            assert st["spans"] == len(batch) and st["dropped_table_full"] == 0
            if cycle == 1:
                if cfg.exp_max_size:
                    _assert_expo_equal(res, batch, cfg.exp_max_size)
                else:
                    assert_red_equal(res, o.series())
                hll, cms = o.window(wid)
                assert np.array_equal(sk.hll, hll) and np.array_equal(sk.cms, cms)
        del cols, res, sk
        free.append(_free(dev))
    drift = free[1] - free[-1]  # > 0: less free memory after cycle 8 than after cycle 2
    print(f"lifecycle[{path}]: free after each destroy (MiB) {[f >> 20 for f in free]}, "
          f"drift cycle 2 -> 8 = {drift} B, steps {sorted(set(np.diff(free).tolist()))}")
    assert drift <= MARGIN, (path, drift, free)
