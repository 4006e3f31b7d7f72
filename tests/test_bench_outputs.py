"""`bench.py --dump-outputs DIR`: the restored frames of the last timed step as float32 .npy, at most 64 MB, sampled at
seeded positions when larger; and a plain run (no --full) prints the headline line only."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_small_output_is_written_whole(tmp_path):
    frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(2, 8, 12, 3), dtype=np.uint8))
    bench.dump_outputs(str(tmp_path / "d"), frames)
    got = np.load(tmp_path / "d" / "restored_frames.npy")
    assert got.dtype == np.float32 and got.shape == frames.shape
    assert np.array_equal(got, frames.numpy().astype(np.float32))


def test_dump_large_output_is_a_fixed_sample_under_the_cap(tmp_path):
    n = (bench.DUMP_SAMPLES // 15 + 1000) * 15
    frames = torch.from_numpy((np.arange(n, dtype=np.int64) % 251).astype(np.uint8).reshape(-1, 5, 3))
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), frames)
    bench.dump_outputs(str(b), frames.clone())
    x, y = np.load(a / "restored_frames.npy"), np.load(b / "restored_frames.npy")
    assert x.dtype == np.float32 and x.ndim == 1 and 0 < x.size <= bench.DUMP_SAMPLES
    assert x.nbytes <= 64 << 20
    assert np.array_equal(x, y)                         # same positions in every run
    assert set(np.unique(x).astype(int)) <= set(range(251))


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu_device, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
           "--frames", "3", "--height", "256", "--width", "384", "--batch", "3", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["higher_is_better"] is True and line["dtype"] == "f16" and line["unit"] == "frames/s"
    assert "hbm_resident" not in line and "roofline" not in line      # measured with --full only
    out = np.load(tmp_path / "restored_frames.npy")
    assert out.dtype == np.float32 and out.shape == (3, 256, 384, 3)
    assert out.min() >= 0 and out.max() <= 255 and np.array_equal(out, np.round(out))
