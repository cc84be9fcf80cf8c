"""bench.py plumbing on CPU: `--gpus N` outside torchrun launches N rank
processes itself (gloo here, --dry-run touches no GPU), they meet in a barrier
and rank 0 reports n_gpus = N with the max over ranks."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT


@pytest.mark.parametrize("n", [1, 2, 3])
def test_bench_self_launches_n_ranks(n):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--dry-run"],
                       capture_output=True, text=True, timeout=240, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout            # only rank 0 prints
    out = json.loads(lines[0])
    assert out["n_gpus"] == n and out["max_rank"] == n - 1
    assert out["backend"] == ("gloo" if n > 1 else None)


def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch):
    """--dump-outputs: float32 .npy per output; an array over the size cap is
    cut to a fixed sample of its (logical NCDHW order) elements, the same
    positions on every call."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 100)
    big = torch.arange(2 * 3 * 4 * 5 * 6, dtype=torch.float32).view(2, 3, 4, 5, 6)
    outs = {"sample": big.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3),   # channels-last strides
            "small": torch.tensor([1.5, -2.0], dtype=torch.bfloat16)}
    bench.dump_outputs(str(tmp_path / "a"), outs)
    bench.dump_outputs(str(tmp_path / "b"), outs)
    assert sorted(os.listdir(tmp_path / "a")) == ["sample.npy", "small.npy"]
    a, b = np.load(tmp_path / "a" / "sample.npy"), np.load(tmp_path / "b" / "sample.npy")
    assert a.dtype == np.float32 and a.shape == (100,)
    assert np.array_equal(a, b)
    idx = a.astype(np.int64)              # the values are their own flat NCDHW positions
    assert np.all(np.diff(idx) > 0) and idx[-1] < big.numel()
    small = np.load(tmp_path / "a" / "small.npy")
    assert small.dtype == np.float32 and small.tolist() == [1.5, -2.0]


def test_cpu_threads_and_model():
    sys.path.insert(0, ROOT)
    import bench
    assert 1 <= bench.cpu_threads() <= (os.cpu_count() or 1)
    assert isinstance(bench.cpu_model(), str)
