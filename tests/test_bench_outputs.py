"""bench.py --dump-outputs on the CPU: the helpers that turn the timed context's arrays into
DIR/<name>.npy (float32 / float64, a fixed seeded sample of rows over DUMP_MAX_ROWS, DUMP_MAX_BYTES
in all), and the option itself through the `--standin` workload.  The GPU path is covered by
tests/test_gpu_bench_outputs.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_rows_types_and_sample():
    import bench
    n = bench.DUMP_MAX_ROWS
    small = np.arange(12, dtype=np.uint8).reshape(3, 4)
    out = bench.dump_rows(small)
    assert out.dtype == np.float32 and np.array_equal(out, small)
    assert bench.dump_rows(np.array([True, False])).dtype == np.float32
    assert bench.dump_rows(np.ones(3, np.float64)).dtype == np.float64
    wide = bench.dump_rows(np.array([1 << 31, 3], np.uint32))          # float32 would round it
    assert wide.dtype == np.float64 and wide[0] == float(1 << 31)
    big = np.arange(3 * n, dtype=np.int32)
    a, b = bench.dump_rows(big), bench.dump_rows(big.copy())
    assert a.shape == (n,) and np.array_equal(a, b)                    # the same rows every time
    assert np.all(np.diff(a) >= 0) and a.max() > 2 * n                 # in index order, over the whole array
    rec = np.zeros(2 * n, np.dtype([("sdf", "<i2"), ("w", "u1"), ("pad", "u1")]))
    rec["sdf"] = np.arange(2 * n) % 30000
    rec["pad"] = 9
    f = bench.dump_fields(rec, ("sdf", "w"))
    assert f.shape == (n, 2) and f[:, 1].max() == 0 and f[:, 0].max() > 0


def test_dump_outputs_budget(tmp_path, monkeypatch):
    import bench
    bench.dump_outputs(str(tmp_path / "a"), {"x": np.zeros((5, 4), np.float32), "y": np.arange(3)})
    assert sorted(os.listdir(tmp_path / "a")) == ["x.npy", "y.npy"]
    assert np.load(tmp_path / "a" / "y.npy").dtype == np.float32
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 64)
    with pytest.raises(AssertionError):
        bench.dump_outputs(str(tmp_path / "b"), {"x": np.zeros(32, np.float32)})


def _standin(out_dir, full=False):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TFUSION_RDZV_DIR", "TFUSION_LAUNCHED"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--standin", "--steps", "2",
           "--dump-outputs", str(out_dir)] + (["--full"] if full else [])
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_standin_dump_outputs_repeat(tmp_path):
    """Two runs with the same arguments write the same arrays; --full is accepted."""
    d = _standin(tmp_path / "a")
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    _standin(tmp_path / "b", full=True)
    a, b = np.load(tmp_path / "a" / "pose.npy"), np.load(tmp_path / "b" / "pose.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4) and np.array_equal(a, b)
    assert np.abs(a[:, :3] @ a[:, :3].T - np.eye(3)).max() < 1e-5       # a tracked pose, not zeros
