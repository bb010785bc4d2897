"""The HIP kernels against the reference's own shared per-element functions, bit for bit.

The expected values are the reference's outputs in tests/golden/stage_pin_<scene>_<case>.bin (layout
and provenance: tests/test_oracle_stage_pin.py), not the oracle's: a misreading shared by the oracle
and a kernel fails here.  The scenes of tests/pin_scenes.py are uploaded into a 96 x 72 context with
the reference's hash sizes (0x100000 buckets, 0x20000 excess entries) and 0x1000 voxel blocks, one
context per scene, and the existing stage entry points run on them: stage_raycast (castRay<false> and
<true>), stage_integrate / tf_scene_integrate_rgb, stage_expected_depths, stage_icp_maps and tf_vis_render_image's five
types on the old raycast.  No device code is added.

The library has no entry point for the point reads (sdf_read), for the allocation request arrays
(alloc_pp) or for checkBlockVisibility alone, so those three cases are compared with the oracle only (tests/test_oracle_stage_pin.py).  Pixels
processPixelICP does not find are expected to be NaN: the reference's device branch, which its host
build cannot show."""
import ctypes

import numpy as np
import pytest

import pin_scenes as P
from parity_util import assert_bit_exact
from test_oracle_stage_pin import RENDER_TYPES, expected_planes, golden, icp_expected, oracle_params

pytestmark = pytest.mark.gpu


class Ctx:
    def __init__(self, name):
        from topfusion_amd import TopFu, default_params
        from topfusion_amd import _lib as L
        self.L, self.name, self.s = L, name, P.scene(name)
        self.g = TopFu(default_params(**oracle_params()))
        self.g.upload(L.TF_BUF_HASH, self.s["hash"])
        self.g.upload(L.TF_BUF_RANGE, P.range_image(name))
        self.load_voxels(0)

    def load_voxels(self, n_visible, visible_ids=()):
        L, g, s = self.L, self.g, self.s
        g.upload(L.TF_BUF_VBA, s["vba"])
        g.upload(L.TF_BUF_VBA_RGB, s["vba_rgb"])
        ids = np.zeros(g.nbytes(L.TF_BUF_VISIBLE_IDS) // 4, np.int32)
        ids[:len(visible_ids)] = visible_ids
        g.upload(L.TF_BUF_VISIBLE_IDS, ids)
        g.upload(L.TF_BUF_VISIBLE_TYPE, np.zeros(P.N_TOTAL, np.uint8))
        g.set_counters(P.N_BLOCKS - 1 - len(s["blocks"]), s["last_excess"], n_visible)


@pytest.fixture(scope="module", params=P.SCENES)
def ctx(request):
    c = Ctx(request.param)
    yield c
    c.g.close()


def test_raycast(ctx):
    g, L, name = ctx.g, ctx.L, ctx.name
    gold = golden(name, "raycast")
    for cam in "ab":
        want = gold[f"points_{cam}"].reshape(P.H, P.W, 4)
        g.upload(L.TF_BUF_VISIBLE_TYPE, np.zeros(P.N_TOTAL, np.uint8))
        g.stage_raycast(ctx.s[f"cam_{cam}"][0], 0)
        assert_bit_exact(f"{name} castRay<false>, camera {cam}", g.raycast_result(), want)
        assert not g.visible_type().any()
        g.stage_raycast(ctx.s[f"cam_{cam}"][0], 1)
        assert_bit_exact(f"{name} castRay<true>, camera {cam}", g.raycast_result(), want)
        vt = g.visible_type()
        assert set(np.unique(vt)) <= {0, 1}
        assert_bit_exact(f"{name} entriesVisibleType, camera {cam}", np.nonzero(vt)[0].astype(np.uint32), gold[f"visible_{cam}"])


def test_integrate(ctx):
    from test_gpu_engines import Pitched, _f, _ok
    g, L, name, s = ctx.g, ctx.L, ctx.name, ctx.s
    gold = golden(name, "integrate")
    lib = L.load()
    intr = np.array(P.intrinsics(), np.float32)
    dbuf, cbuf = Pitched(P.H, P.W, np.float32), Pitched(P.H, P.W, np.uint8, 4)
    cbuf.put(P.rgb_image(name))
    try:
        for frame, (pose, dists, vis) in enumerate(P.integrate_inputs(name)):
            want_vba, want_rgb = expected_planes(name, gold, frame)
            for colour in (False, True):
                ctx.load_voxels(len(vis), vis)
                if colour:
                    dbuf.put(dists)
                    _ok(lib.tf_scene_integrate_rgb(g._h, _f(intr), _f(pose.reshape(12)), dbuf.ptr, dbuf.step,
                                                   ctypes.c_void_p(cbuf.ptr), cbuf.step), "tf_scene_integrate_rgb")
                else:
                    g.upload(L.TF_BUF_DISTS, dists)
                    g.stage_integrate(pose)
                got = g.vba()
                assert_bit_exact(f"{name} frame {frame} sdf", got["sdf"], want_vba["sdf"])
                assert_bit_exact(f"{name} frame {frame} w_depth", got["w"], want_vba["w"])
                assert_bit_exact(f"{name} frame {frame} colour plane", g.vba_rgb(), want_rgb if colour else s["vba_rgb"])
    finally:                                    # the context serves the module: leave it as the fixture made it
        dbuf.free()
        cbuf.free()
        ctx.load_voxels(0)


def test_expected_depths(ctx):
    g, L, name, s = ctx.g, ctx.L, ctx.name, ctx.s
    gold = golden(name, "expected_depths")
    vis = P.expected_depths_list(name)
    try:
        ctx.load_voxels(len(vis), vis)
        g.stage_expected_depths(s["cam_d"][1])
        got, n = g.range_image(), g.stats()["noTotalBlocks"]
    finally:
        g.upload(L.TF_BUF_RANGE, P.range_image(name))
        ctx.load_voxels(0)
    assert_bit_exact(f"{name} CreateExpectedDepths range image", got, gold["range"].reshape(P.H, P.W, 2))
    assert n == len(gold["block_z"]) // 2


def test_icp_maps(ctx):
    g, name = ctx.g, ctx.name
    want_pts, want_nrm = icp_expected(golden(name, "pixels"))
    g.stage_raycast(ctx.s["cam_a"][0], 1)                   # CreateICPMaps: castRay<true>, then renderICP_device<false>
    g.stage_icp_maps(ctx.s["cam_a"][0])
    assert_bit_exact(f"{name} raycast of CreateICPMaps", g.raycast_result(),
                     golden(name, "raycast")["points_a"].reshape(P.H, P.W, 4))
    pts, nrm = g.prev_maps(0)
    assert_bit_exact(f"{name} processPixelICP points", pts, want_pts)
    assert_bit_exact(f"{name} processPixelICP normals", nrm, want_nrm)


def test_render_types_on_old_raycast(ctx):
    from test_gpu_engines import Pitched, _f, _ok
    g, L, name = ctx.g, ctx.L, ctx.name
    gold = golden(name, "pixels")
    lib = L.load()
    intr = np.array(P.intrinsics(), np.float32)
    c2w = ctx.s["cam_a"][0]
    g.stage_raycast(c2w, 0)
    assert_bit_exact(f"{name} raycast", g.raycast_result(), golden(name, "raycast")["points_a"].reshape(P.H, P.W, 4))
    img = Pitched(P.H, P.W, np.uint8, 4)
    for key, t in RENDER_TYPES:
        g.upload(L.TF_BUF_GREY, np.zeros((P.H, P.W, 4), np.uint8))       # drawPixelNormal leaves alpha as it was
        _ok(lib.tf_vis_render_image(g._h, _f(intr), _f(c2w.reshape(12)), t, 0, img.ptr, img.step), "tf_vis_render_image")
        assert_bit_exact(f"{name} RenderImage type {t} ({key})", img.get(), gold[key].reshape(P.H, P.W, 4))
    img.free()
