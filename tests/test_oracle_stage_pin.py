"""The CPU oracle's stage functions against the reference's own shared per-element functions.

tests/golden/stage_pin_<scene>_<case>.bin hold what the reference's _CPU_AND_GPU_CODE_ inline
functions (RepresentationAccess.hpp, VisualisationEngine_Shared.hpp, SceneReconstructionEngine.hpp,
compiled for the host from the reference tree by oracle/ref_pin/ref_pin_stages.cpp) compute over the
scenes of tests/pin_scenes.py.  Here the oracle runs over the same scenes and must agree bit for bit;
tests/test_gpu_stage_pin.py does the same with the HIP kernels.  Only tests/golden and the repository
are read, except by the freshness test, which runs where the reference tree exists.

Golden layout (pin files, pin_scenes.read_pin: named little-endian arrays).  Every file has
  crc     u32[3]   CRC32 of the scene's hash, VBA and colour-plane bytes (asserted first)
  counts  i32[]    branch hits counted by the pin program (pin_scenes.check_coverage)
sdf_read, n = 4096 points of pin_scenes.sdf_points, "2" = (fresh IndexCache, carried IndexCache):
  uninterp f32[n,2], vm i32[n,2]       readFromSDF_float_uninterpolated and its vmIndex
  interp f32[n,2]                       readFromSDF_float_interpolated
  conf_sdf f32[n,2], conf f32[n,2]      readWithConfidenceFromSDF_float_interpolated, its confidence
  normal f32[n,3]                       computeSingleNormalFromSDF
  colour u8[n,4]                        drawPixelColour on the Voxel_s_rgb copy of the scene
  counts: missing block, found in a bucket entry, in an excess entry, carried-cache hits, +1
  neighbours in another block all present, some missing, negative coordinates, exact integers; a +1
  neighbour in a block with no entry, in a swapped-out block, in a block chained in an excess entry
raycast, cameras a and b, range image pin_scenes.range_image:
  points_a / points_b f32[H,W,4]        castRay<.., false>'s pt_out (castRay<.., true>'s is identical)
  visible_a / visible_b u32[]           the entries castRay<.., true> marks in entriesVisibleType
  counts per camera: found, missed, rays whose range has min >= max, entries marked, rays with steps in
  missing blocks, rays that took the march's interpolated read (the march walked again beside the call)
integrate, frames 0, 1 and 2 of pin_scenes.integrate_inputs, each applied to the scene as it is:
  voxel_idx<f> u32[], voxel<f> u32[]    changed voxels: index, sdf (low 16 bits) | w_depth << 16
  colour_idx<f> u32[], colour<f> u32[]  changed colours: index, r | g << 8 | b << 16 | w_color << 24
  counts per frame: list entries with ptr < 0, voxels behind the camera, outside the image, on no
  depth, eta < -mu, updated, eta == -mu, eta / mu > 1, already at maxW, colour gate passed, colours changed,
  updated with pt_image exactly on the edge of the window (1, W - 2, H - 2)
alloc_pp, camera a, the dists image pin_scenes.alloc_inputs (the pixel loop run forwards and backwards gave the same):
  entry_idx u32[k], entry_flags u8[k,2], entry_coords i16[k,4]  every entry buildHashAllocAndVisibleTypePP wrote:
                                        index, entriesAllocType, entriesVisibleType, blockCoords
  counts: entries with alloc type 1, type 2, found visible (type 1), found swapped out (type 2), found in an excess
  entry, requests at negative block coordinates; pixels with depth <= 0, under the near limit, over the far limit,
  pixels walked, of them with noSteps == 1 (none: the walk is 2 mu = one block long, so noSteps is 2 or 3)
visibility, n = 4096 blocks of pin_scenes.visibility_blocks, camera b:
  flags u8[n,4]                         isVisible, isVisibleEnlarged of checkBlockVisibility<false>, then <true>
  counts: visible, enlarged only, invisible, first corner behind the camera
expected_depths, camera d, the visible list pin_scenes.expected_depths_list:
  entry_valid u8[n], entry_box i16[n,4], entry_z f32[n,2]  ProjectSingleBlock per list entry: accepted, upperLeft x, y,
                                        lowerRight x, y, zRange (zeros where rejected or ptr < 0)
  block_corners i16[b,4], block_z f32[b,2]  the rendering blocks ProjectSingleBlock + CreateRenderingBlocks make, in
                                        entry order: upperLeft x, y, lowerRight x, y; zRange min, max (b = noTotalBlocks)
  range f32[H,W,2]                      the range image after the FAR_AWAY / VERY_CLOSE memset and fillBlocks_device
  counts: list entries with ptr < 0, rejected, accepted projections, accepted with some corners behind the camera,
  boxes touching the left, top, right, bottom image side, boxes of more than one rendering block
pixels, on points_a:
  icp_idx u32[m], icp f32[m,6]          processPixelICP<false, false>: found pixels, point xyz, normal xyz (both w = 1)
  grey, grey_imagenormals, normal, confidence, colour  u8[H,W,4]: processPixelGrey,
  processPixelGrey_ImageNormals<true, false>, processPixelNormal, processPixelConfidence, processPixelColour
  counts: lit pixels of the six outputs; doPlus1 of computeNormalAndAngle<true, false> taken, not taken

Host / device differences of the reference that the goldens cannot show:
processPixelICP writes 0 on the host where the device writes a quiet NaN (its __CUDA_ARCH__ branch),
so pixels not found are expected to be NaN; computeUpdatedVoxelDepthInfo's fx * x / z is an IEEE
division on the host, while the oracle and the kernels follow the CUDA build's --prec-div=false with
(fx * x) * (1 / z): the chosen inputs give the same voxels either way (the test would show any other).
"""
import os
import subprocess

import numpy as np
import pytest

import pin_scenes as P
from parity_util import assert_bit_exact

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/tfusion/include"
RENDER_TYPES = (("grey", 0), ("grey_imagenormals", 1), ("colour", 2), ("normal", 3), ("confidence", 4))


def golden(scene, case):
    d = P.read_pin(P.golden_path(scene, case))
    assert_bit_exact(f"{scene} {case}: scene CRC32", d["crc"], P.scene(scene)["crc"])
    return d


def oracle_params(**kw):
    fx, fy, cx, cy = P.intrinsics()
    return dict(cols=P.W, rows=P.H, fx=float(fx), fy=float(fy), cx=float(cx), cy=float(cy), voxel_rgb=1,
                n_buckets=P.N_BUCKETS, n_excess=P.N_EXCESS, n_blocks=P.N_BLOCKS, **kw)


def expected_planes(scene, g, frame):
    """The scene's voxels and colour plane after integrate frame `frame`, by the reference."""
    s = P.scene(scene)
    vba, rgb = s["vba"].copy(), s["vba_rgb"].copy()
    idx, word = g[f"voxel_idx{frame}"], g[f"voxel{frame}"]
    vba["sdf"][idx] = (word & 0xFFFF).astype(np.uint16).view(np.int16)
    vba["w"][idx] = word >> 16
    rgb[g[f"colour_idx{frame}"]] = g[f"colour{frame}"]
    return vba, rgb


def icp_expected(g):
    """processPixelICP's maps: the stored pixels, a quiet NaN everywhere else (the device branch)."""
    pts = np.full((P.W * P.H, 4), np.nan, np.float32)
    nrm = np.full((P.W * P.H, 4), np.nan, np.float32)
    icp = g["icp"].reshape(-1, 6)
    pts[g["icp_idx"], :3], pts[g["icp_idx"], 3] = icp[:, :3], 1.0
    nrm[g["icp_idx"], :3], nrm[g["icp_idx"], 3] = icp[:, 3:], 1.0
    return pts.reshape(P.H, P.W, 4), nrm.reshape(P.H, P.W, 4)


@pytest.fixture(scope="module", params=P.SCENES)
def loaded(request, oracle_mod):
    """(scene name, an Oracle holding the scene and the supplied range image)."""
    name = request.param
    s = P.scene(name)
    o = oracle_mod.Oracle(oracle_mod.default_params(**oracle_params()))
    o.upload_hash(s["hash"])
    o.upload_vba(s["vba"], s["vba_rgb"])
    o.upload_range_image(P.range_image(name))
    o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], 0)
    return name, o


@pytest.mark.parametrize("scene", P.SCENES)
@pytest.mark.parametrize("case", P.CASES)
def test_coverage(scene, case):
    """The committed goldens meet the coverage conditions they were written under."""
    P.check_coverage(case, golden(scene, case))
    assert os.path.getsize(P.golden_path(scene, case)) <= P.MAX_GOLDEN_BYTES


def test_voxel_rgb_size_is_the_recorded_one():
    """ref_pin_stages.cpp static_asserts sizeof(Voxel_s_rgb) == REF_PIN_SIZEOF_VOXEL_S_RGB: the value
    ref_pin_colour.bin records (its first float)."""
    import re
    recorded = np.fromfile(os.path.join(P.GOLDEN, "ref_pin_colour.bin"), "<f4", 1)[0]
    with open(os.path.join(ROOT, "oracle", "ref_pin", "ref_pin_stages.cpp")) as f:
        m = re.search(r"#define REF_PIN_SIZEOF_VOXEL_S_RGB (\d+)", f.read())
    assert m and float(m.group(1)) == recorded


def test_scene_properties():
    """What the scenes are meant to contain."""
    s = P.scene("sphere")
    assert (s["blocks"][:, 0] < 0).any() and (s["blocks"][:, 1] < 0).any() and (s["blocks"][:, 0] > 0).any()
    assert set(np.unique(s["vba"]["w"][:len(s["blocks"]) * 512])) == {1, 5, 100}
    assert (s["hash"]["ptr"] == -1).sum() >= 16
    pl = P.scene("plane")
    assert len(pl["blocks"]) <= P.N_BLOCKS and (pl["hash"]["ptr"] == -1).sum() >= 16
    assert (pl["blocks"].min(0)[:2] < 0).all() and (pl["blocks"].max(0)[:2] > 0).all()
    assert np.ptp(pl["blocks"][:, 2]) >= 16                                    # oblique: the slab spans many z blocks
    r = P.scene("random")
    h = r["hash"]
    assert len(r["blocks"]) <= P.N_BLOCKS and len(s["blocks"]) <= P.N_BLOCKS
    assert set(np.unique(r["vba"]["w"])) == {0, 1, 5, 100}
    for v in (0, 32767, -32767):
        assert (r["vba"]["sdf"] == v).mean() > 0.05
    # chains of a bucket entry and three excess entries, with swapped-out and unallocated members
    pos = r["special"].reshape(-1, 4, 3)
    hi = P.synth.hash_index(pos[..., 0], pos[..., 1], pos[..., 2], P.N_BUCKETS)
    assert np.all(hi == hi[:, :1])
    mid_swapped = mid_free = 0
    for b, first in zip(hi[:, 0], pos[:, 0]):
        walk = list(P.chain(h, P.N_BUCKETS, first))
        assert len(walk) == 4 and walk[0] == b
        mid_swapped += any(h["ptr"][w] == -1 for w in walk[1:3])
        mid_free += any(h["ptr"][w] < -1 for w in walk[1:3])
    assert mid_swapped >= 3 and mid_free == 1
    live = h["ptr"][h["ptr"] >= 0]
    assert len(np.unique(live)) == len(live) and not np.array_equal(live, np.sort(live))     # shuffled VBA pointers


def test_sdf_read(loaded):
    name, o = loaded
    g = golden(name, "sdf_read")
    pts = P.sdf_points(name)
    for k, tag in enumerate(("fresh cache", "carried cache")):
        u, vm, i, cs, cf = o.sdf_read(pts, carried=k)
        assert_bit_exact(f"{name} vmIndex, {tag}", vm, g["vm"].reshape(-1, 2)[:, k])
        assert_bit_exact(f"{name} readFromSDF_float_uninterpolated, {tag}", u, g["uninterp"].reshape(-1, 2)[:, k])
        assert_bit_exact(f"{name} readFromSDF_float_interpolated, {tag}", i, g["interp"].reshape(-1, 2)[:, k])
        assert_bit_exact(f"{name} readWithConfidenceFromSDF_float_interpolated, {tag}", cs, g["conf_sdf"].reshape(-1, 2)[:, k])
        assert_bit_exact(f"{name} confidence, {tag}", cf, g["conf"].reshape(-1, 2)[:, k])
    assert_bit_exact(f"{name} computeSingleNormalFromSDF", o.normal_from_sdf(pts), g["normal"].reshape(-1, 3))
    assert_bit_exact(f"{name} drawPixelColour", o.colour_at(pts), g["colour"].reshape(-1, 4))


def test_raycast(loaded):
    name, o = loaded
    g = golden(name, "raycast")
    s = P.scene(name)
    for cam in "ab":
        want = g[f"points_{cam}"].reshape(P.H, P.W, 4)
        o.upload_visible_type(np.zeros(P.N_TOTAL, np.uint8))
        o.raycast(s[f"cam_{cam}"][0], 0)
        assert_bit_exact(f"{name} castRay<false>, camera {cam}", o.raycast_result(), want)
        assert not o.visible_type().any()
        o.raycast(s[f"cam_{cam}"][0], 1)
        assert_bit_exact(f"{name} castRay<true>, camera {cam}", o.raycast_result(), want)
        vt = o.visible_type()
        assert set(np.unique(vt)) <= {0, 1}
        assert_bit_exact(f"{name} entriesVisibleType, camera {cam}", np.nonzero(vt)[0].astype(np.uint32), g[f"visible_{cam}"])


def test_integrate(loaded):
    name, o = loaded
    g = golden(name, "integrate")
    s = P.scene(name)
    rgb = P.rgb_image(name)
    for frame, (pose, dists, vis) in enumerate(P.integrate_inputs(name)):
        want_vba, want_rgb = expected_planes(name, g, frame)
        for colour in (False, True):
            o.upload_vba(s["vba"], s["vba_rgb"])
            o.upload_visible_ids(vis)
            o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], len(vis))
            o.integrate(pose, dists, rgb if colour else None)
            got = o.vba()
            assert_bit_exact(f"{name} frame {frame} sdf", got["sdf"], want_vba["sdf"])
            assert_bit_exact(f"{name} frame {frame} w_depth", got["w"], want_vba["w"])
            assert_bit_exact(f"{name} frame {frame} colour plane", o.vba_rgb(), want_rgb if colour else s["vba_rgb"])
    o.upload_vba(s["vba"], s["vba_rgb"])
    o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], 0)


def test_alloc_pp(loaded):
    name, o = loaded
    g = golden(name, "alloc_pp")
    s = P.scene(name)
    pose, dists = P.alloc_inputs(name)
    try:
        alloc, vis, coords = o.alloc_requests(pose, dists)
        assert_bit_exact(f"{name} hash untouched", o.hash().view(np.uint8), s["hash"].view(np.uint8))
    finally:
        o.upload_visible_type(np.zeros(P.N_TOTAL, np.uint8))
        o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], 0)
    want_alloc, want_vis, want_coords = np.zeros(P.N_TOTAL, np.uint8), np.zeros(P.N_TOTAL, np.uint8), np.zeros((P.N_TOTAL, 4), np.int16)
    want_alloc[g["entry_idx"]], want_vis[g["entry_idx"]] = g["entry_flags"].reshape(-1, 2).T
    want_coords[g["entry_idx"]] = g["entry_coords"].reshape(-1, 4)
    assert_bit_exact(f"{name} entriesAllocType", alloc, want_alloc)
    assert_bit_exact(f"{name} entriesVisibleType", vis, want_vis)
    assert_bit_exact(f"{name} blockCoords", coords, want_coords)
    assert g["counts"][10] == 0                  # no pixel with noSteps == 1 in the reference's run


def test_visibility(loaded):
    name, o = loaded
    g = golden(name, "visibility")
    flags = g["flags"].reshape(-1, 4)
    vis, enl = o.block_visibility(P.scene(name)["cam_b"][1], P.visibility_blocks(name))
    assert_bit_exact(f"{name} checkBlockVisibility<false> isVisible", vis, flags[:, 0])
    assert_bit_exact(f"{name} checkBlockVisibility<true> isVisible", vis, flags[:, 2])
    assert_bit_exact(f"{name} checkBlockVisibility<true> isVisibleEnlarged", enl, flags[:, 3])
    assert_bit_exact(f"{name} checkBlockVisibility<false> isVisibleEnlarged", vis, flags[:, 1])


def fill_blocks(g):
    """fillBlocks_device over the golden's rendering-block list: min / max per covered pixel."""
    r = np.empty((P.H, P.W, 2), np.float32)
    r[..., 0], r[..., 1] = P.FAR_AWAY, P.VERY_CLOSE
    for (x0, y0, x1, y1), (z0, z1) in zip(g["block_corners"].reshape(-1, 4), g["block_z"].reshape(-1, 2)):
        assert 0 <= x0 <= x1 < P.W and 0 <= y0 <= y1 < P.H and x1 - x0 < 16 and y1 - y0 < 16
        r[y0:y1 + 1, x0:x1 + 1, 0] = np.minimum(r[y0:y1 + 1, x0:x1 + 1, 0], z0)
        r[y0:y1 + 1, x0:x1 + 1, 1] = np.maximum(r[y0:y1 + 1, x0:x1 + 1, 1], z1)
    return r


def test_expected_depths(loaded):
    """The oracle's block projection per list entry against ProjectSingleBlock's; the golden's rendering
    blocks are CreateRenderingBlocks' split of those boxes in entry order and fill the golden's range image;
    the oracle's range image and block count against the golden's."""
    name, o = loaded
    g = golden(name, "expected_depths")
    s = P.scene(name)
    want = g["range"].reshape(P.H, P.W, 2)
    assert_bit_exact(f"{name} fillBlocks_device over the block list", fill_blocks(g), want)
    vis = P.expected_depths_list(name)
    valid, box, z = o.project_blocks(s["cam_d"][1], vis)
    assert_bit_exact(f"{name} ProjectSingleBlock accepted", valid, g["entry_valid"])
    assert_bit_exact(f"{name} ProjectSingleBlock box", box, g["entry_box"].reshape(-1, 4))
    assert_bit_exact(f"{name} ProjectSingleBlock zRange", z, g["entry_z"].reshape(-1, 2))
    split = [(x0, y0, min(x0 + 15, x1), min(y0 + 15, y1), z0, z1)
             for (X0, Y0, x1, y1), (z0, z1) in zip(box[valid > 0].tolist(), z[valid > 0].tolist())
             for y0 in range(Y0, y1 + 1, 16) for x0 in range(X0, x1 + 1, 16)]
    assert [list(t[:4]) for t in split] == g["block_corners"].reshape(-1, 4).tolist()
    assert_bit_exact(f"{name} rendering blocks' zRange", np.array([t[4:] for t in split], np.float32), g["block_z"].reshape(-1, 2))
    o.upload_visible_ids(vis)
    o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], len(vis))
    o.expected_depths(s["cam_d"][1])
    got, n = o.range_image(), o.counters()["noTotalBlocks"]
    o.upload_range_image(P.range_image(name))
    o.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], 0)
    assert_bit_exact(f"{name} CreateExpectedDepths range image", got, want)
    assert n == len(g["block_z"]) // 2


def test_pixels(loaded):
    name, o = loaded
    g = golden(name, "pixels")
    c2w = P.scene(name)["cam_a"][0]
    o.upload_raycast_result(golden(name, "raycast")["points_a"])
    pts, nrm = o.render_icp(c2w)
    want_pts, want_nrm = icp_expected(g)
    assert_bit_exact(f"{name} processPixelICP points", pts, want_pts)
    assert_bit_exact(f"{name} processPixelICP normals", nrm, want_nrm)
    assert_bit_exact(f"{name} render_grey", o.render_grey(c2w), g["grey"].reshape(P.H, P.W, 4))
    for key, t in RENDER_TYPES:
        assert_bit_exact(f"{name} RenderImage type {t} ({key})", o.render_type(c2w, t), g[key].reshape(P.H, P.W, 4))


@pytest.mark.skipif(not os.path.isdir(REF), reason="the reference tree is not on this machine")
def test_goldens_are_fresh(tmp_path):
    """Where the reference tree exists: both pin programs, rebuilt from it by the Makefile's own recipe
    into a temporary directory, write the committed goldens byte for byte (cases a build without clang's
    HIP mode leaves out are not compared)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(P.GOLDEN, "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref", f"REF_OUT={tmp_path / '_ref'}"],
                       capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    out = tmp_path / "out"
    out.mkdir()
    subprocess.run([str(tmp_path / "_ref" / "ref_pin"), str(out)], check=True, capture_output=True)
    mg.run_stage_pin(str(tmp_path / "_ref" / "ref_pin_stages"), str(out))
    names = sorted(os.listdir(out))
    want = sorted(os.path.basename(P.golden_path(s, c)) for s in P.SCENES for c in P.CASES)
    assert set(n for n in names if n.startswith("stage_pin_")) <= set(want)
    if os.path.exists("/opt/rocm/lib/llvm/bin/clang++"):
        assert [n for n in names if n.startswith("stage_pin_")] == want
    assert len([n for n in names if n.startswith("ref_pin_")]) == 6
    for n in names:
        with open(out / n, "rb") as a, open(os.path.join(P.GOLDEN, n), "rb") as b:
            assert a.read() == b.read(), f"{n} differs from the committed golden"
