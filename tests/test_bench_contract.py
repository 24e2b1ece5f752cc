"""bench.py host logic on CPU: traffic summaries are picked by workload, and the
CPU-baseline worker (the oracle port, bench.py's cpu_baseline leg) reports a
rate.  The timed GPU steps themselves run only on the GPU box."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


@pytest.mark.parametrize("workload,fname", [("c2", "traffic.json"), ("c4", "traffic_c4.json")])
def test_traffic_summary_matches_workload(workload, fname):
    path = os.path.join(ROOT, "profiles", fname)
    traffic, src = bench.load_traffic(path, workload)
    assert src == os.path.join("profiles", fname)
    assert traffic > 44 * 10_000_000 * 0.9  # at least the algorithmic bytes (minus noise)


def test_traffic_summary_of_another_workload_is_not_used():
    path = os.path.join(ROOT, "profiles", "traffic_c4.json")
    assert bench.load_traffic(path, "c4zipf") == (None, None)
    assert bench.load_traffic(os.path.join(ROOT, "profiles", "missing.json"), "c2") == (None, None)


def test_cpu_worker_reports_a_rate():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--cpu-worker", "1",
                        "--cpu-seconds", "0.2"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["spans"] >= 2_000_000 and r["seconds"] > 0


def _red(n, seed=3):
    from spanagg.engine import RedResult
    rng = np.random.default_rng(seed)
    kh = np.sort(rng.integers(1, 2**64 - 1, n, dtype=np.uint64))
    bc = rng.integers(0, 2**40, (n, 17), dtype=np.uint64)
    sum_ns = rng.integers(0, 2**50, n, dtype=np.uint64)
    return RedResult(kh, bc, bc.sum(axis=1), sum_ns, sum_ns / 1e6)


def test_dump_outputs_writes_the_flush_columns_exactly(tmp_path):
    """--dump-outputs: every column of the flush result and the sketches as
    float32/float64 .npy files; u64 key ids survive as two 32-bit halves."""
    from spanagg.engine import SketchResult
    red = _red(1500)
    rng = np.random.default_rng(4)
    sk = [SketchResult(170_000_000 + w, rng.integers(0, 50, (20, 1 << 14)).astype(np.uint8),
                       rng.integers(0, 2**32 - 1, (4, 2048)).astype(np.uint32)) for w in range(3)]
    bench.dump_outputs(str(tmp_path / "out"), red, sk)
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= bench.DUMP_BUDGET_BYTES
    assert "series_index" not in got
    kh = (got["key_hash_hi"].astype(np.uint64) << np.uint64(32)) | got["key_hash_lo"].astype(np.uint64)
    assert np.array_equal(kh, red.key_hash)
    for f in ("bucket_counts", "calls", "sum_ns"):
        assert np.array_equal(got[f].astype(np.uint64), getattr(red, f)), f
    assert np.array_equal(got["sum"], red.sum)
    assert np.array_equal(got["hll"], np.stack([s.hll for s in sk]))
    assert np.array_equal(got["cms"], np.stack([s.cms for s in sk]))
    assert got["window_id"].tolist() == [s.window_id for s in sk]


def test_dump_outputs_writes_an_exponential_flush(tmp_path):
    """c2expo's flush (ExpoResult): the scalar columns exactly, the per-series
    bucket arrays padded with zeros to the widest series."""
    from spanagg.engine import ExpoResult
    u64, f64, i32 = (lambda *v: np.array(v, dtype=np.uint64)), (lambda *v: np.array(v, dtype=np.float64)), \
        (lambda *v: np.array(v, dtype=np.int32))
    red = ExpoResult(u64(5, 2**63 + 9, 2**64 - 1), u64(6, 1, 0), u64(1, 0, 0), u64(7_000_000, 3, 0),
                     f64(7.0, 3e-6, 0.0), f64(0.0, 3e-6, 0.0), f64(4.5, 3e-6, 0.0), i32(3, 20, -10), i32(-7, 12, 0),
                     [u64(1, 0, 4), u64(1), u64()])
    bench.dump_outputs(str(tmp_path), red, [])
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert all(a.dtype == np.float64 for a in got.values())
    kh = (got["key_hash_hi"].astype(np.uint64) << np.uint64(32)) | got["key_hash_lo"].astype(np.uint64)
    assert np.array_equal(kh, red.key_hash)
    for f in ("count", "zero_count", "sum_ns", "sum", "min", "max", "scale", "offset"):
        assert np.array_equal(got[f], getattr(red, f).astype(np.float64)), f
    assert got["buckets"].tolist() == [[1, 0, 4], [1, 0, 0], [0, 0, 0]]
    assert "bucket_counts" not in got and "hll" not in got


def test_dump_outputs_samples_the_same_rows_under_the_budget(tmp_path, monkeypatch):
    """Over the byte budget the per-series columns keep a seeded sample of rows,
    the same rows on every run, named by series_index."""
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 100_000)
    red = _red(4000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), red, [])
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(x.nbytes for x in a.values()) <= 100_000
    idx = a["series_index"].astype(np.int64)
    assert 0 < len(idx) < 4000 and (np.diff(idx) > 0).all()
    assert np.array_equal(a["calls"].astype(np.uint64), red.calls[idx])
    assert np.array_equal(a["bucket_counts"].astype(np.uint64), red.bucket_counts[idx])


@pytest.mark.parametrize("world", [2, 3, 8])
def test_bench_batches_sit_in_their_trace_id_shard(world):
    """bench.py at N ranks: every span of a rank's batch and of each of its
    trace-id variants is owned by that rank under spanagg.dist.shard_of, and
    spans of one trace stay together (equal ids map to equal ids)."""
    import torch
    from spanagg.dist import shard_of
    rng = np.random.default_rng(world)
    w0 = torch.from_numpy(rng.integers(0, 2**63, 20000, dtype=np.int64))
    w1 = torch.from_numpy(rng.integers(0, 2**64 - 1, 20000, dtype=np.uint64).view(np.int64))
    w1[1000:1010] = w1[0]  # one trace with several spans
    for rank in range(world):
        for v0, v1 in bench.trace_variants(w0, w1, 3, seed=5, rank=rank, world=world):
            u = v1.numpy().view(np.uint64)
            assert (shard_of(u, world) == rank).all()
            assert (u[1000:1010] == u[0]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 3, 8])
def test_bench_trace_id_shards_on_device(world):
    """The same sharding on device-resident columns (bench.py applies it to
    cuda tensors): every span of each variant lands on its rank."""
    import torch
    from spanagg.dist import shard_of
    rng = np.random.default_rng(world)
    w0 = torch.from_numpy(rng.integers(0, 2**63, 50000, dtype=np.int64)).cuda()
    w1 = torch.from_numpy(rng.integers(0, 2**64 - 1, 50000, dtype=np.uint64).view(np.int64)).cuda()
    for rank in range(world):
        for _, v1 in bench.trace_variants(w0, w1, 3, seed=9, rank=rank, world=world):
            assert v1.is_cuda
            assert (shard_of(v1.cpu().numpy().view(np.uint64), world) == rank).all()


_RANK_SCRIPT = r'''
import json, os, sys, time
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
with open(os.path.join(sys.argv[1], f"rank{rank}.json"), "w") as f:
    json.dump({k: os.environ[k] for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                          "SPANAGG_BENCH_LAUNCHER")}, f)
fail = int(sys.argv[2])
if fail >= 0:
    if rank == fail:
        sys.exit(3)
    time.sleep(120)      # the others wait, as in a collective the failed rank never joins
if rank == 0:
    print(json.dumps({"n_gpus": world}))
'''


@pytest.mark.parametrize("n", [2, 4])
def test_launch_ranks_spawns_n_rank_processes(tmp_path, n, capfd):
    """bench.py --gpus N without torch.distributed.run: launch_ranks starts N
    children with the torch.distributed.run environment (distinct RANK /
    LOCAL_RANK, one WORLD_SIZE, one loopback rendezvous), and rank 0's stdout
    is what the parent prints."""
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT)
    rc = bench.launch_ranks(n, [str(tmp_path), "-1"], script=str(script), timeout=120)
    assert rc == 0
    envs = [json.loads((tmp_path / f"rank{i}.json").read_text()) for i in range(n)]
    assert sorted(int(e["RANK"]) for e in envs) == list(range(n))
    assert all(e["RANK"] == e["LOCAL_RANK"] and e["WORLD_SIZE"] == str(n) for e in envs)
    assert len({e["MASTER_PORT"] for e in envs}) == 1 and envs[0]["MASTER_ADDR"] == "127.0.0.1"
    assert all(e["SPANAGG_BENCH_LAUNCHER"].startswith("bench.py") for e in envs)
    out = capfd.readouterr().out.strip().splitlines()
    assert json.loads(out[-1]) == {"n_gpus": n}


def test_launch_ranks_propagates_a_rank_failure(tmp_path):
    """A rank that fails ends the job with its exit code, and the ranks left
    waiting for it are stopped (not left to hang until a time limit)."""
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT)
    t0 = __import__("time").monotonic()
    rc = bench.launch_ranks(3, [str(tmp_path), "1"], script=str(script), timeout=100)
    assert rc == 3
    assert __import__("time").monotonic() - t0 < 60


def test_bench_self_launch_without_gpu_fails_loudly():
    """`bench.py --gpus 2` on a box without a GPU: both rank children fail and
    the parent returns non-zero (it neither hangs nor prints a line)."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--spans", "1000",
                        "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode != 0
    assert not p.stdout.strip()


@pytest.mark.gpu
def test_bench_self_launch_two_ranks_one_device(tmp_path):
    """The scaling line's launch path on a one-GPU box: a bare `bench.py
    --gpus 2` (no outer launcher) starts two ranks on cuda:0 over gloo; the
    line reports n_gpus 2, the backend, a world size of 2 and both ranks.
    --dump-outputs writes rank 0's merged flush: both ranks' spans."""
    env = dict(os.environ, SPANAGG_BENCH_ONE_DEVICE="1")
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--spans", "1000000",
                        "--steps", "4", "--warmup", "1", "--settle", "1", "--soak-s", "0", "--sub", "",
                        "--no-cpu-baseline", "--host-otlp-spans", "0", "--h2d-reps", "0",
                        "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=110, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["n_gpus"] == 2 and r["calls_check"]
    d = r["distributed"]
    assert d["world_size"] == 2 and d["backend"] == "gloo" and d["launcher"].startswith("bench.py")
    assert sorted(x["rank"] for x in d["per_rank"]) == [0, 1]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    launches = 1 + 1 + 1 + 2 * 3 + 4  # cold, settle, warm-up, 2 * n_iso, timed
    assert int(got["calls"].sum()) == 2 * launches * 1_000_000
    assert np.array_equal(got["bucket_counts"].sum(axis=1), got["calls"])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_its_outputs(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W`: the line carries the
    headline figure and none of the --full legs, and --dump-outputs writes the
    flush of every launch so far (calls add up to launches x spans) with the
    window sketches."""
    spans, steps, warmup, settle = 200_000, 5, 2, 2
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--spans", str(spans), "--settle", str(settle),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=110)
    assert p.returncode == 0, p.stderr[-3000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["steps"] == steps and r["calls_check"] and r["higher_is_better"] and r["dtype"] == "u64"
    assert r["unit"] == "spans/s" and r["ms_per_step"] > 0
    assert abs(r["value"] - spans / (r["ms_per_step"] * 1e-3)) <= 1e-6 * r["value"]
    for leg in ("c4", "c4zipf", "c2expo", "c2_graph", "hll_filter_off", "host_buffer_ingest", "cpu_baseline",
                "cpu_baseline_multicore", "host_otlp", "group"):
        assert leg not in r, leg
    assert r["sustained"] is None and "kernel_ms" not in r["roofline"]
    got = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    launches = 1 + settle + warmup + 2 * max(3, steps // 5) + steps
    assert int(got["calls"].sum()) == launches * spans
    assert np.array_equal(got["bucket_counts"].sum(axis=1), got["calls"])
    assert got["hll"].shape[1:] == (20, 1 << 14) and got["hll"].max() > 0
    assert got["cms"].shape[1:] == (4, 2048) and len(got["window_id"]) == len(got["hll"])
