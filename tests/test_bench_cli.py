"""bench.py launch plumbing on the CPU (VERDICT r2 Missing #2): `--gpus N` without a launcher
spawns N rank processes (torch.distributed.run, 127.0.0.1), a launcher's WORLD_SIZE must equal
--gpus, and every rank holds the pixel shard DESIGN.md §5 plans (whole tile columns of the tiled
stored order).  --dry-run stops before anything touches a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=env, timeout=timeout,
                       cwd=ROOT)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    return p.returncode, (json.loads(lines[-1]) if lines else None), p


def test_single_rank_plan():
    rc, d, _ = _run(["--dry-run"])
    assert rc == 0 and d["world"] == 1 and d["mode"] == "single GPU"
    assert d["shards"] == [[0, 4096 * 4096]]


@pytest.mark.parametrize("n,workload", [(2, "c4"), (3, "c3")])
def test_gpus_n_spawns_n_ranks(n, workload):
    rc, d, p = _run(["--gpus", str(n), "--dry-run", "--workload", workload])
    assert rc == 0, p.stderr[-2000:]
    N = 4096 if workload == "c4" else 2048
    assert d["world"] == n and d["mode"] == "pixel-sharded"
    assert [r["rank"] for r in d["ranks"]] == list(range(n))
    assert [r["local_rank"] for r in d["ranks"]] == list(range(n))     # one GPU per rank
    sh = [tuple(r["shard"]) for r in d["ranks"]]
    assert sh[0][0] == 0 and sh[-1][1] == N * N
    assert all(a[1] == b[0] for a, b in zip(sh, sh[1:]))
    assert all((hi - lo) % (4 * N) == 0 for lo, hi in sh)               # whole 4 x N tile columns
    sizes = [hi - lo for lo, hi in sh]
    assert max(sizes) - min(sizes) <= 4 * N


@pytest.mark.parametrize("workload,dtype", [("c4", "f64"), ("c5", "f32"), ("c5m", "f32"), ("c3gcv", "f64")])
def test_plan_carries_dtype(workload, dtype):
    """configs[4] (c5/c5m) is fp32 on N GPUs: the plan every rank follows names that dtype
    (bench.py build_shard cuts the fp32 shards; main() refuses operators of another dtype)."""
    rc, d, p = _run(["--gpus", "2", "--dry-run", "--workload", workload])
    assert rc == 0, p.stderr[-2000:]
    assert d["dtype"] == dtype and d["mode"] == "pixel-sharded"


def test_replicas_plan():
    rc, d, _ = _run(["--gpus", "2", "--dry-run", "--replicas"])
    assert rc == 0 and d["mode"] == "replicas" and d["world"] == 2


def test_world_size_must_match_gpus():
    rc, d, p = _run(["--gpus", "2", "--dry-run"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert rc == 2 and d is None
    assert "WORLD_SIZE=4" in p.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hgm_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: every output as float64 <name>.npy; a short x whole, a long one as the same
    seeded sample (values and positions) on every call; later ranks of a multi-GPU run add
    _rank<r>."""
    import numpy as np
    bench = _bench_module()
    small = {"x": np.arange(7, dtype=np.float32), "error_norm": np.ones(3), "niters": [3]}
    bench.dump_outputs(str(tmp_path / "a"), small, 0, 1)
    assert sorted(os.listdir(tmp_path / "a")) == ["error_norm.npy", "niters.npy", "x.npy"]
    x = np.load(tmp_path / "a" / "x.npy")
    assert x.dtype == np.float64 and np.array_equal(x, np.arange(7))
    assert np.array_equal(np.load(tmp_path / "a" / "niters.npy"), [3.0])
    bench.dump_outputs(str(tmp_path / "a"), small, 1, 2)
    assert os.path.exists(tmp_path / "a" / "x_rank1.npy")

    n = bench.DUMP_X_MAX + 5
    big = {"x": np.sqrt(np.arange(n, dtype=np.float64))}
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big, 0, 1)
    assert sorted(os.listdir(tmp_path / "b")) == ["x_sample.npy", "x_sample_index.npy"]
    idx = np.load(tmp_path / "b" / "x_sample_index.npy")
    xs = np.load(tmp_path / "b" / "x_sample.npy")
    assert idx.dtype == xs.dtype == np.float64 and idx.size == xs.size == bench.DUMP_X_MAX
    assert np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(xs, big["x"][idx.astype(np.int64)])
    assert np.array_equal(idx, np.load(tmp_path / "c" / "x_sample_index.npy"))
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 64 * 10**6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeatable_outputs(tmp_path):
    """A plain run (C2, the smallest workload) times exactly --steps steps, leaves cpu_baseline to
    --full, and --dump-outputs writes the last step's outputs: x, both histories, niters.  Two runs
    with the same arguments start from identical inputs, so their outputs agree to the parity bar
    of the suite (1e-10 relative: fp64 sums whose order may differ between runs, over 20 Arnoldi
    steps)."""
    import numpy as np
    got = []
    for d in ("a", "b"):
        rc, line, p = _run(["--gpus", "1", "--workload", "c2", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / d)])
        assert rc == 0, p.stderr[-2000:]
        assert line["steps"] == 3 and line["warmup"] == 1 and line["cpu_baseline"] is None
        assert line["dtype"] == "f64" and line["higher_is_better"] is True
        # value = iterations of the 3 timed 20-iteration solves over their time
        assert abs(line["value"] * line["ms_per_step"] * 1e-3 / 20 - 1) < 1e-3
        assert sorted(os.listdir(tmp_path / d)) == ["error_norm.npy", "niters.npy", "residual_norm.npy", "x.npy"]
        got.append({f: np.load(tmp_path / d / f) for f in os.listdir(tmp_path / d)})
    a, b = got
    assert a["x.npy"].shape == (512 * 512,) and a["niters.npy"][0] == 20
    assert a["error_norm.npy"].shape == a["residual_norm.npy"].shape == (20,)
    for f in a:
        assert a[f].dtype == np.float64 and np.all(np.isfinite(a[f]))
        dev = np.linalg.norm(a[f] - b[f]) / np.linalg.norm(a[f])
        print(f"{f}: run-to-run deviation {dev:.2e}")
        assert dev < 1e-10, (f, dev)
    assert b["residual_norm.npy"][-1] == line["monitors"]["residual_norm_last"]   # the second run's line


def test_tile_column_shards_host():
    from hgmres.dist import tile_column_shards
    for N, w in ((4096, 8), (2048, 8), (512, 4), (64, 3)):
        sh = tile_column_shards(N, w, 4)
        assert len(sh) == w and sh[0][0] == 0 and sh[-1][1] == N * N
        assert all((hi - lo) % (4 * N) == 0 for lo, hi in sh)
    with pytest.raises(ValueError):
        tile_column_shards(8, 3, 4)
