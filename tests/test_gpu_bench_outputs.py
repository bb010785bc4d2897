"""bench.py on the GPU, as every later change runs it: a plain `--gpus 1 --steps K --warmup W` run
does the headline's work only, `--dump-outputs DIR` writes what the timed context holds after its
last step -- the same arrays from run to run, and the ones a caller of tf_process_frames on the
same frames receives -- and `--full` still fills the fields that moved behind it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

STEPS, WARMUP, F, W, H = 2, 1, 32, 640, 480
NAMES = ["counters", "grey", "hash", "ok", "pose", "raycast", "voxels"]


def _bench(*extra):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "TFUSION_RDZV_DIR", "TFUSION_LAUNCHED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--profile-every", "1"] + [str(e) for e in extra],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench("--dump-outputs", d / "a"), d / "a"


def _load(path):
    assert sorted(os.listdir(path)) == [n + ".npy" for n in NAMES]
    return {n: np.load(path / (n + ".npy")) for n in NAMES}


def test_plain_line(plain):
    d = plain[0]
    assert d["steps"] == STEPS and d["warmup"] == WARMUP and d["n_gpus"] == 1
    assert d["unit"] == "frames/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["metric"].startswith("fused frames/sec @640x480, 5 mm voxel hash")
    assert d["ms_per_step"] == pytest.approx(1000.0 * F / d["value"], rel=1e-3)     # one step = F frames
    assert d["roofline"]["kernel"] == "k_icp_frame" and d["roofline"]["avg_launch_ms"] > 0
    # nothing that takes a run of its own
    for k in ("cpu_baseline", "other_algebra", "c1", "per_call_frames_per_sec", "per_call_batched_same_frames",
              "icp_integrate_ms_per_frame", "hbm_stream_copy_GBs", "stage_breakdown"):
        assert d[k] is None, k
    assert d["stage_ms_per_frame"] == {} and list(d["roofline_stages"]) == ["icp"]


def test_dump_is_what_a_caller_receives(plain):
    """The dumped arrays against this process's own context over the same 96 frames."""
    import bench
    from topfusion_amd import TopFu, default_params, synth
    out = _load(plain[1])
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64 * 1000 * 1000
    n = (WARMUP + STEPS) * F
    dev = bench.orbit_frames(n, W, H, 7)
    fx, fy, cx, cy = synth.intrinsics(W, H)
    g = TopFu(default_params(cols=W, rows=H, fx=fx, fy=fy, cx=cx, cy=cy, voxelSize=0.005))
    for s in range(WARMUP + STEPS):
        ok = g.process_frames(dev.ptr + s * F * W * H * 2, F)
    st = g.stats()
    assert np.array_equal(out["ok"], ok.astype(np.float32)) and out["ok"].shape == (F,)
    assert np.array_equal(out["pose"], g.getCameraPose())
    assert list(out["counters"]) == [st["lastFreeBlockId"], st["lastFreeExcessListId"], st["noVisibleEntries"]]
    assert np.array_equal(out["grey"], g.frame_grey().reshape(-1, 4).astype(np.float32))
    assert np.array_equal(out["raycast"], g.raycast_result().reshape(-1, 4), equal_nan=True)
    assert np.array_equal(out["hash"], bench.dump_rows(bench.dump_fields(g.hash(), ("x", "y", "z", "offset", "ptr"))))
    assert np.array_equal(out["voxels"], bench.dump_rows(bench.dump_fields(g.vba(), ("sdf", "w"))))
    assert out["hash"].shape == (bench.DUMP_MAX_ROWS, 5) and out["voxels"].shape == (bench.DUMP_MAX_ROWS, 2)
    assert (out["hash"][:, 4] >= 0).sum() > 100 and out["voxels"][:, 1].max() > 0    # a fused scene, not an empty one
    g.close()
    dev.free()


def test_dump_repeats_and_full_fills_the_rest(plain, tmp_path):
    """A second process with the same arguments writes the same arrays; with --full it also reports
    the breakdown, the per-call rates, C1, the other algebra and the copy rate."""
    d = _bench("--full", "--no-cpu-baseline", "--dump-outputs", tmp_path / "b")
    a, b = _load(plain[1]), _load(tmp_path / "b")
    for n in NAMES:
        assert a[n].dtype == b[n].dtype and np.array_equal(a[n], b[n], equal_nan=True), n
    assert d["steps"] == STEPS and d["per_call_frames_per_sec"] > 0 and d["c1"]["gpu_ms_per_frame"] > 0
    assert d["other_algebra"]["frames_per_sec"] > 0 and d["hbm_stream_copy_GBs"] > 0
    assert d["stage_ms_per_frame"]["icp"] > 0 and d["stage_ms_per_frame"]["integrate"] > 0
    assert set(d["roofline_stages"]) == {"icp", "raycast_icp", "integrate"}
