"""bench.py's multi-rank launch, on CPU (no GPU call: OCFFM_BENCH_DRY=1 stops
every rank after the gloo rendezvous and one all-reduce).

The driver's scale command is `python bench.py --gpus N`: without torchrun's
environment the script must start N ranks itself, and rank 0 must report
n_gpus = N with every rank accounted for.  Under torchrun (WORLD_SIZE set)
it must not spawn again, and a --gpus that disagrees with WORLD_SIZE is an
error rather than a mislabelled line.  Also --dump-outputs' writer on
made-up arrays.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(args, env_extra=None, timeout=240):
    env = dict(os.environ, OCFFM_BENCH_DRY="1", MASTER_ADDR="127.0.0.1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    env.update(env_extra or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env,
                          cwd=REPO)


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_flag_spawns_n_ranks(n):
    r = _run(["--gpus", str(n)])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout  # rank 0 alone prints
    assert lines[0] == {"n_gpus": n, "ranks_seen": n, "launcher": "spawn"}


def test_single_gpu_does_not_spawn():
    r = _run(["--gpus", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1]) == {"n_gpus": 1, "ranks_seen": 1, "launcher": "none"}


def test_torchrun_world_is_used():
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", "29631", BENCH, "--gpus", "2"],
                       capture_output=True, text=True, timeout=240, cwd=REPO,
                       env=dict(os.environ, OCFFM_BENCH_DRY="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert lines == [{"n_gpus": 2, "ranks_seen": 2, "launcher": "torchrun"}]


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: every array whole below the size limit; past it the
    same seeded sample of each array's elements from run to run, within the limit."""
    import importlib.util

    import numpy as np
    monkeypatch.setattr(sys, "argv", [BENCH])
    spec = importlib.util.spec_from_file_location("bench_under_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(5)
    arrays = {"W_00": rng.standard_normal(1000), "H_00": rng.standard_normal(3001), "W_01": np.arange(7.0)}
    bench.dump_outputs(str(tmp_path / "whole"), arrays, np.float64)
    for name, a in arrays.items():
        got = np.load(tmp_path / "whole" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4008 * 4 // 4)  # a quarter of the 4008 float32 elements
    bench.dump_outputs(str(tmp_path / "a"), arrays, np.float32)
    bench.dump_outputs(str(tmp_path / "b"), arrays, np.float32)
    kept = 0
    for name, a in arrays.items():
        got = np.load(tmp_path / "a" / (name + ".npy"))
        assert got.dtype == np.float32 and np.array_equal(got, np.load(tmp_path / "b" / (name + ".npy")))
        assert got.size == max(1, a.size // 4)
        pos = np.searchsorted(np.sort(a.astype(np.float32)), got)  # elements of a, each at most once
        assert np.array_equal(np.sort(a.astype(np.float32))[pos], got) and np.unique(pos).size == got.size
        kept += got.nbytes
    assert kept <= 4008


def test_gpus_disagreeing_with_world_is_an_error():
    r = _run(["--gpus", "4"], env_extra={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE" in (r.stderr + r.stdout)
