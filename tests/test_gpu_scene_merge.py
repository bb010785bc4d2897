"""The map merge on the GPU (tf_map_merge and the layers above it, topfusion_amd/csrc/tf_scene_ckpt.hip) against the
serial restatement (tests/scene_merge_ref.py) bit for bit: the made pair with either offset, with exactly the free
slots it needs and in staging chunks of 1, 3 and more blocks than the file has; as a twin of a context that got the
restatement's state by upload (free views, mesh, further frames: the block grid); over a live sequence; its refusals;
twice."""
import os
import subprocess

import numpy as np
import pytest

import scene_ckpt_ref as R
import scene_map_ref as MR
import scene_merge_ref as G
import test_gpu_scene_ckpt as C
import test_gpu_scene_map as T
from topfusion_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = T.W, T.H
OFFSETS = ((0, 0, 0), G.MADE_OFFSET)
BLOCK = 8 * 0.005                                        # metres per block at the made pair's voxel size


def _ctx(**kw):
    return T._ctx(False, **dict(G.MADE, vis_capacity=4096, max_render_blocks=4096, **kw))


def _bytes(g):
    """Everything the download entry points give, as bytes."""
    s = C._state(g)
    out = {k: np.ascontiguousarray(v).tobytes() for k, v in s.items() if isinstance(v, np.ndarray) and k != "params"}
    out["maps"] = b"".join(np.ascontiguousarray(m).tobytes() for m in s["maps"])
    out["counters"] = s["counters"]
    return out


def _assert_state(tag, got, want):
    for k in ("hash", "vba", "visType", "allocList", "excessList", "pose"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (tag, k)
    assert got["counters"] == want["counters"], (tag, got["counters"], want["counters"])
    n = want["counters"]["noVisibleEntries"]
    assert np.asarray(got["visibleIds"])[:n].tobytes() == np.asarray(want["visibleIds"], np.int32)[:n].tobytes(), (tag, "visibleIds")
    assert all(np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes() for a, b in zip(got["maps"], want["maps"])), (tag, "maps")


_shared = {}


def _made(tmp_path_factory):
    """(target, file state, the file's path), the restatement's results per offset: made once."""
    if not _shared:
        target, file = G.made_pair()
        path = tmp_path_factory.mktemp("merge") / "made.tfscene"
        path.write_bytes(R.pack(file))
        _shared.update(target=target, file=file, path=path, want={off: G.merge(target, file, off) for off in OFFSETS})
    return _shared


def _merged(m, off, target=None):
    g = _ctx()
    C._upload_state(g, m["target"] if target is None else target)
    return g, g.merge_map(m["path"], off)


# ---- 1. against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", OFFSETS)
def test_against_restatement(tmp_path_factory, off):
    m = _made(tmp_path_factory)
    want, report = m["want"][off]
    assert report["records_combined"] > 0 and report["records_inserted"] > 0 and report["records_revived"] > 0 and report["records_skipped"] > 0
    g, got = _merged(m, off)
    assert got == report
    _assert_state(("made", off), C._state(g), want)
    g.close()
    # exactly the free slots it needs: both lists end at -1
    B, X = report["blocks_used"], report["excess_used"]
    exact = G.with_free(m["target"], B, X)
    want_exact, _ = G.merge(exact, m["file"], off)
    g, got = _merged(m, off, exact)
    assert got == report
    s = C._state(g)
    _assert_state(("exact", off), s, want_exact)
    assert s["counters"]["lastFreeBlockId"] == -1 and s["counters"]["lastFreeExcessListId"] == -1
    g.close()


@pytest.mark.parametrize("chunk", [1, 3, 100000])
def test_chunks(tmp_path_factory, monkeypatch, chunk):
    """TFUSION_CKPT_CHUNK_BLOCKS is read when the context is created: staging chunks of 1 and 3 blocks (a ragged
    last one) and one larger than the file give the same bytes."""
    m = _made(tmp_path_factory)
    assert len(G.carried(m["file"])[0]) % 3 != 0 and len(G.carried(m["file"])[0]) < 100000
    monkeypatch.setenv("TFUSION_CKPT_CHUNK_BLOCKS", str(chunk))
    off = G.MADE_OFFSET
    g, got = _merged(m, off)
    assert got == m["want"][off][1]
    _assert_state(("chunk", chunk), C._state(g), m["want"][off][0])
    g.close()


# ---- 2. the twin ----------------------------------------------------------------------------------------------------------
def _look(block, back):
    """A camera `back` blocks behind block position `block`, looking along +z."""
    c2w = np.eye(4, dtype=np.float32)
    c2w[:3, 3] = (np.asarray(block, np.float64) - (0, 0, back)) * BLOCK
    return c2w


def test_twin(tmp_path_factory):
    """The merged context beside one that got merge()'s state by upload (its block grid is rebuilt from the hash):
    the same free-view raycast and image from a pose at the table's middle and from one that looks at the blocks the
    offset put outside the block grid, the same mesh, the same tables, verdicts and poses over further frames.  Both
    views see merged blocks: neither shows what the unmerged target shows."""
    m = _made(tmp_path_factory)
    off = G.MADE_OFFSET
    want, _ = m["want"][off]
    a, _ = _merged(m, off)
    b, before = _ctx(), _ctx()
    C._upload_state(b, want)
    C._upload_state(before, m["target"])
    _, pos, _, _ = G.carried(m["file"], off)
    outside = pos[((pos < -G.GRID_HALF) | (pos >= G.GRID_HALF)).any(axis=1)]
    far = outside[outside[:, 2] < -G.GRID_HALF]
    assert len(far) >= 5
    poses = (_look((0, 0, 0), 45), _look(far[:, :3].mean(axis=0), 12))
    for k, c2w in enumerate(poses):
        shots = []
        for g in (a, b, before):
            with g.view(64, 48) as v:
                image = v.render(c2w)
                shots.append((v.raycast_result().tobytes(), image.tobytes(), int((v.raycast_result()[..., 3] > 0).sum())))
        assert shots[0][:2] == shots[1][:2], k
        assert shots[0][2] > 50 and shots[0][0] != shots[2][0], (k, shots[0][2], shots[2][2])
    mesh = a.mesh()
    assert len(mesh) > 0 and mesh.tobytes() == b.mesh().tobytes() and mesh.tobytes() != before.mesh().tobytes()
    # further frames: fused at known poses, then tracked
    n = 4
    seq = synth.orbit_sequence(n, W, H, seed=7)
    w2c = synth.world_to_camera_rt(*(np.stack(x) for x in zip(*(synth.orbit_pose(k) for k in range(n)))))
    dev = synth.DeviceStream(2, W, H)
    dev.upload(seq[:2])
    ra, rb = a.fuse_frames(dev.ptr, w2c[:2]), b.fuse_frames(dev.ptr, w2c[:2])
    assert ra.tobytes() == rb.tobytes()
    assert _bytes(a) == _bytes(b)
    for k in range(2, n):
        assert bool(a(seq[k])) == bool(b(seq[k])), k
        assert a.getCameraPose().tobytes() == b.getCameraPose().tobytes(), k
        assert _bytes(a) == _bytes(b), k
    assert a.mesh().tobytes() == b.mesh().tobytes()
    dev.free()
    for g in (a, b, before):
        g.close()


# ---- 3. a live sequence ---------------------------------------------------------------------------------------------------
LIVE = dict(n_buckets=4096, n_excess=2048, n_blocks=8192, voxelSize=0.0075)


def test_live_sequence(tmp_path):
    """A fuses frames 0..k of the orbit, B (other tables) frames k..2k; B saved and merged into A is the restatement's
    merge of the two downloaded states: blocks both saw combine, B's own are inserted."""
    k = 3
    seq = synth.orbit_sequence(2 * k + 1, W, H, seed=7, deg_per_frame=4.0)
    w2c = synth.world_to_camera_rt(*(np.stack(x) for x in zip(*(synth.orbit_pose(i, 4.0) for i in range(2 * k + 1)))))
    dev = synth.DeviceStream(2 * k + 1, W, H)
    dev.upload(seq)
    a = T._ctx(False, **LIVE)
    b = T._ctx(False, **dict(LIVE, n_buckets=1024, n_excess=4096, n_blocks=4096))
    a.fuse_frames(dev.ptr, w2c[:k + 1])
    b.fuse_frames(dev.frame_ptr(k), w2c[k:])
    path = tmp_path / "b.tfscene"
    b.save_map(path)
    sa, sb = C._state(a), C._state(b)
    want, report = G.merge(sa, sb)
    assert report["records_combined"] > 20 and report["records_inserted"] > 20
    assert a.merge_map(path) == report
    _assert_state("live", C._state(a), want)
    dev.free()
    a.close()
    b.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(tmp_path_factory, tmp_path):
    from topfusion_amd import TfError, _lib as L
    m = _made(tmp_path_factory)
    path, file, target = m["path"], m["file"], m["target"]
    need = m["want"][(0, 0, 0)][1]
    B, X = need["blocks_used"], need["excess_used"]

    def refused(g, file_path, status, report=None, off=(0, 0, 0)):
        before = _bytes(g)
        with pytest.raises(TfError) as e:
            g.merge_map(file_path, off)
        assert e.value.status == status, (e.value.status, status)
        assert e.value.report == report
        assert _bytes(g) == before

    for nb_free, ne_free in ((B - 1, X + 5), (B + 5, X - 1)):       # one block, one excess slot too few
        g = _ctx()
        C._upload_state(g, G.with_free(target, nb_free, ne_free))
        refused(g, path, L.TF_CAPACITY, need)
        g.close()
    g = _ctx()
    C._upload_state(g, target)
    truncated = tmp_path / "truncated.tfscene"
    truncated.write_bytes(path.read_bytes()[:-1])
    refused(g, truncated, L.TF_INVALID_ARG)
    refused(g, tmp_path / "missing.tfscene", L.TF_INVALID_ARG)
    for key, value in (("voxelSize", 0.006), ("mu", 0.03), ("maxW", 50)):
        p = file["params"].copy()
        p[key] = value
        other = tmp_path / f"{key}.tfscene"
        other.write_bytes(R.pack(dict(file, params=p)))
        refused(g, other, L.TF_INVALID_ARG)
    dup = dict(file, hash=file["hash"].copy())                       # two carried records of one position
    k = np.flatnonzero(dup["hash"]["ptr"] >= 0)
    for f in "xyz":
        dup["hash"][f][k[-1]] = dup["hash"][f][k[0]]
    twice = tmp_path / "dup.tfscene"
    twice.write_bytes(R.pack(dup))
    refused(g, twice, L.TF_INVALID_ARG)
    _, pos, _, _ = G.carried(file)
    refused(g, path, L.TF_INVALID_ARG, off=(32767 - int(pos[:, 0].max()) + 1, 0, 0))
    refused(g, path, L.TF_INVALID_ARG, off=(0, -32768 - int(pos[:, 1].min()) - 1, 0))
    v2 = tmp_path / "v2.tfmap"                                       # a version-2 file, a colour file
    v2.write_bytes(MR.pack(MR.tiny_state()))
    refused(g, v2, L.TF_INVALID_ARG)
    colour = tmp_path / "colour.tfscene"
    colour.write_bytes(R.pack(R.tiny_state(voxel_rgb=1)))
    refused(g, colour, L.TF_INVALID_ARG)
    g.close()
    for kw in (dict(use_swapping=1, swap_transfer_blocks=16), dict(voxel_rgb=1)):     # a swapping, a colour context
        g = _ctx(**kw)
        before = T._state(g)
        with pytest.raises(TfError) as e:
            g.merge_map(path)
        assert e.value.status == L.TF_INVALID_ARG and e.value.report is None
        after = T._state(g)
        for key in ("hash", "vba", "visType", "allocList", "excessList"):
            assert after[key].tobytes() == before[key].tobytes(), key
        assert after["counters"] == before["counters"]
        g.close()


# ---- 5. determinism -------------------------------------------------------------------------------------------------------
def test_determinism_and_a_second_merge(tmp_path_factory):
    m = _made(tmp_path_factory)
    off = G.MADE_OFFSET
    a, ra = _merged(m, off)
    b, rb = _merged(m, off)
    assert ra == rb and _bytes(a) == _bytes(b)
    want2, report2 = G.merge(m["want"][off][0], m["file"], off)
    carried = len(G.carried(m["file"])[0])
    assert report2 == dict(records_combined=carried, records_inserted=0, records_revived=0, records_skipped=report2["records_skipped"],
                           blocks_used=0, excess_used=0)
    assert a.merge_map(m["path"], off) == report2
    _assert_state("twice", C._state(a), want2)
    a.close()
    b.close()


# ---- the layers above -----------------------------------------------------------------------------------------------------
def test_map_merge_check_app(tmp_path):
    """apps/map_merge_check: two Scenes over the two halves of a walk through the C++ engine layer, the second saved
    and merged into the first (Scene::mergeMap): combined and inserted records, counters that fell by the report, a
    mesh that grew, a second merge that only combines."""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "apps"), "map_merge_check"], check=True)
    r = subprocess.run([os.path.join(ROOT, "apps", "map_merge_check"), "12", str(tmp_path / "b.tfscene"), str(tmp_path / "a.ply")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "MATCH" in r.stdout and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    assert os.path.getsize(tmp_path / "a.ply") > 1000
