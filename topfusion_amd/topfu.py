"""Python mirror of the reference's pipeline API (tfusion/include/tfusion/topfu.hpp:28-110)
over the C-ABI of libtfusion_hip.so.

    params = TopFuParams.default_params()     # topfu.cpp:12-53
    topfu = TopFu(params)                     # topfu.cpp:55-84
    ok = topfu(depth)                         # operator(), topfu.cpp:161-330
    img = topfu.renderImage()                 # topfu.cpp:332-377
    pose = topfu.getCameraPose()              # topfu.cpp:154-159
    topfu.reset()                             # topfu.cpp:141-152

`depth` is a uint16 (rows, cols) numpy array (host; uploaded like cuda::Depth::upload)
or a device pointer (int) to uint16 millimetres on the context's device.
"""
import ctypes

import numpy as np

from . import _lib as L

HASH_DTYPE = np.dtype([("x", "<i2"), ("y", "<i2"), ("z", "<i2"), ("pad", "<i2"), ("offset", "<i4"), ("ptr", "<i4")])
VOXEL_DTYPE = np.dtype([("sdf", "<i2"), ("w", "u1"), ("pad", "u1")])


class TopFuParams:
    """TopFuParams: construct with default_params() and override attributes."""

    @staticmethod
    def default_params(**kw):
        return L.default_params(**kw)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _rt(m):
    a = np.ascontiguousarray(np.asarray(m, np.float32)[:3, :4] if np.ndim(m) == 2 else np.asarray(m, np.float32))
    return a.reshape(12)


class View:
    """A free view of a TopFu's map (tf_view, include/tfusion_hip.h): its own size, visible list, range image,
    raycast result and image.  Rendering through it leaves the tracker's state and output untouched.  Poses are
    3x4 / 4x4 [R|t]: `c2w` camera -> world, `w2c` world -> camera; `intr` (fx, fy, cx, cy), None: the context's.
    `whole` is the view's reading (tf_set_view_reading): False, the blocks in the VBA; True, on a swapping TopFu,
    the blocks of the GlobalCache as well.
    Created by TopFu.view(); close() (or the with statement) releases it early, the TopFu's close() at the latest."""

    def __init__(self, owner, cols, rows, vis_capacity=0, max_render_blocks=0, whole=False):
        self._owner = owner
        self._h = None
        vp = L.TfViewParams(int(cols), int(rows), int(vis_capacity), int(max_render_blocks))
        h = ctypes.c_void_p()
        L.check(L.load().tf_view_create(owner._h, ctypes.byref(vp), ctypes.byref(h)), "tf_view_create")
        self._h = h
        L.check(L.load().tf_view_get_params(h, ctypes.byref(vp)), "tf_view_get_params")
        self.W, self.H = vp.cols, vp.rows
        self.vis_capacity, self.max_render_blocks = vp.vis_capacity, vp.max_render_blocks
        self.needed = 0               # entries the last find_visible found (also when it raised TF_CAPACITY)
        owner._views.append(self)
        if whole:
            self.whole = True

    @property
    def whole(self):
        r = ctypes.c_int(0)
        L.check(L.load().tf_get_view_reading(self._handle(), ctypes.byref(r)), "tf_get_view_reading")
        return r.value == L.TF_VIEW_WHOLE

    @whole.setter
    def whole(self, on):
        L.check(L.load().tf_set_view_reading(self._handle(), L.TF_VIEW_WHOLE if on else L.TF_VIEW_RESIDENT), "tf_set_view_reading")

    def close(self):
        if self._h and self._owner._h:          # (a closed TopFu has released its views already)
            L.load().tf_view_destroy(self._h)
        self._h = None
        if self in self._owner._views:
            self._owner._views.remove(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _intr(intr):
        return None if intr is None else np.ascontiguousarray(intr, np.float32).reshape(4)

    def _handle(self):
        if not self._h or not self._owner._h:
            raise RuntimeError("the view (or its TopFu) is closed")
        return self._h

    def find_visible(self, w2c, intr=None):
        """FindVisibleBlocks: the number of entries in the view's list.  TfError(TF_CAPACITY) when more qualify
        than vis_capacity (`needed` then holds the number)."""
        i, n = self._intr(intr), ctypes.c_int(0)
        s = L.load().tf_view_find_visible(self._handle(), None if i is None else _ptr(i), _ptr(_rt(w2c)), ctypes.byref(n))
        self.needed = n.value
        L.check(s, "tf_view_find_visible")
        return n.value

    def expected_depths(self, w2c, intr=None):
        i = self._intr(intr)
        L.check(L.load().tf_view_expected_depths(self._handle(), None if i is None else _ptr(i), _ptr(_rt(w2c))),
                "tf_view_expected_depths")

    def raycast(self, c2w, intr=None):
        i = self._intr(intr)
        L.check(L.load().tf_view_raycast(self._handle(), None if i is None else _ptr(i), _ptr(_rt(c2w))), "tf_view_raycast")

    def shade(self, c2w, type=0, intr=None):
        """The pixel stage of `type` on the view's raycast result: (rows, cols, 4) uint8."""
        i = self._intr(intr)
        L.check(L.load().tf_view_shade(self._handle(), None if i is None else _ptr(i), _ptr(_rt(c2w)), int(type), None, 0),
                "tf_view_shade")
        return self.image()

    def render(self, c2w, type=0, intr=None):
        """The map from camera -> world pose `c2w`: (rows, cols, 4) uint8."""
        i = self._intr(intr)
        L.check(L.load().tf_view_render(self._handle(), None if i is None else _ptr(i), _ptr(_rt(c2w)), int(type), None, 0),
                "tf_view_render")
        return self.image()

    def icp_maps(self, c2w, intr=None):
        """renderICP on the view's raycast result: (points, normals), (rows, cols, 4) float32 each."""
        out = [np.empty((self.H, self.W, 4), np.float32) for _ in range(2)]
        hip = L.hip_runtime()
        devs = [ctypes.c_void_p() for _ in range(2)]
        try:
            for d, o in zip(devs, out):
                if hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(o.nbytes)) != 0:
                    raise L.TfError(L.TF_OOM, "hipMalloc (view maps)")
            i = self._intr(intr)
            L.check(L.load().tf_view_icp_maps(self._handle(), None if i is None else _ptr(i), _ptr(_rt(c2w)), devs[0], 0,
                                              devs[1], 0), "tf_view_icp_maps")
            for d, o in zip(devs, out):
                if hip.hipMemcpy(_ptr(o), d, ctypes.c_size_t(o.nbytes), 2) != 0:      # hipMemcpyDeviceToHost
                    raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (view maps)")
        finally:
            for d in devs:
                if d:
                    hip.hipFree(d)
        return out[0], out[1]

    def _download(self, which, dtype, shape):
        buf = np.empty(shape, dtype)
        L.check(L.load().tf_view_download(self._handle(), which, _ptr(buf), buf.nbytes), "tf_view_download")
        return buf

    def stats(self):
        nv, nb = ctypes.c_int(0), ctypes.c_int(0)
        L.check(L.load().tf_view_stats(self._handle(), ctypes.byref(nv), ctypes.byref(nb)), "tf_view_stats")
        return {"noVisibleEntries": nv.value, "noTotalBlocks": nb.value}

    def visible_ids(self):
        return self._download(L.TF_VIEW_VISIBLE_IDS, np.int32, (self.vis_capacity,))[:self.stats()["noVisibleEntries"]]

    def range_image(self):
        return self._download(L.TF_VIEW_RANGE, np.float32, (self.H, self.W, 2))

    def raycast_result(self):
        return self._download(L.TF_VIEW_RAYCAST, np.float32, (self.H, self.W, 4))

    def image(self):
        return self._download(L.TF_VIEW_IMAGE, np.uint8, (self.H, self.W, 4))


class TopFu:
    """tfusion::TopFu on one MI355X (one HIP stream per instance)."""

    def __init__(self, params=None, device=None, **kw):
        lib = L.load()
        if device is not None:
            L.check(lib.tf_set_device(int(device)), "tf_set_device")
        self.params_ = params if params is not None else L.default_params(**kw)
        h = ctypes.c_void_p()
        L.check(lib.tf_create(ctypes.byref(self.params_), ctypes.byref(h)), "tf_create")
        self._h = h
        self.W, self.H = self.params_.cols, self.params_.rows
        self.n_total = self.params_.n_buckets + self.params_.n_excess
        self._framed = False
        self._views = []

    def close(self):
        if getattr(self, "_h", None):
            L.load().tf_destroy(self._h)      # releases the views still alive
            self._h = None
            for v in list(getattr(self, "_views", [])):
                v._h = None
            self._views = []

    def view(self, cols=None, rows=None, vis_capacity=0, max_render_blocks=0, whole=False):
        """A free view of the map (View): cols x rows (None: the context's), a visible list of vis_capacity entries
        (0: n_buckets + n_excess) and a tile cap of max_render_blocks (0: the context's).  whole: the view reads the
        GlobalCache of a swapping TopFu as well as its VBA (View.whole)."""
        return View(self, self.W if cols is None else cols, self.H if rows is None else rows, vis_capacity, max_render_blocks,
                    whole)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self):
        return self.params_

    # -- TopFu API ----------------------------------------------------------------------
    def __call__(self, depth, pitch=0, rgb=None):
        """TopFu::operator()(depth, image): returns the frame's bool (False = ICP failed, scene
        reset).  rgb (voxel_rgb contexts): the frame's uchar4 (rows, cols, 4) image -- a host array
        with a host depth, a device pointer with a device depth."""
        lib = L.load()
        pose = np.zeros(12, np.float32)
        if isinstance(depth, int):
            if rgb is None:
                s = lib.tf_process_frame(self._h, ctypes.c_void_p(depth), pitch, _ptr(pose), None)
            else:
                s = lib.tf_process_frame_rgb(self._h, ctypes.c_void_p(depth), pitch, ctypes.c_void_p(int(rgb)), 0,
                                             _ptr(pose), None)
        else:
            d = np.ascontiguousarray(depth, np.uint16)
            assert d.shape == (self.H, self.W), d.shape
            if rgb is None:
                s = lib.tf_process_frame_host(self._h, _ptr(d), self.W * 2, _ptr(pose), None)
            else:
                c = np.ascontiguousarray(rgb, np.uint8)
                assert c.shape == (self.H, self.W, 4), c.shape
                s = lib.tf_process_frame_rgb_host(self._h, _ptr(d), self.W * 2, _ptr(c), self.W * 4, _ptr(pose),
                                                  None)
        L.check(s, "tf_process_frame", allow=(L.TF_OK, L.TF_ICP_FAIL))
        self._framed = True
        return s == L.TF_OK

    def process_frames(self, dev_frames, n, stride=None, rgb_frames=None, rgb_stride=None):
        """Runs n device-resident frames (and, voxel_rgb, their device-resident RGB images);
        returns the per-frame bools."""
        ok = np.zeros(n, np.int32)
        stride = stride if stride is not None else self.W * self.H * 2
        if rgb_frames is None:
            L.check(L.load().tf_process_frames(self._h, ctypes.c_void_p(dev_frames), stride, n, _ptr(ok)),
                    "tf_process_frames")
        else:
            rs = rgb_stride if rgb_stride is not None else self.W * self.H * 4
            L.check(L.load().tf_process_frames_rgb(self._h, ctypes.c_void_p(dev_frames), stride,
                                                   ctypes.c_void_p(int(rgb_frames)), rs, n, _ptr(ok)),
                    "tf_process_frames_rgb")
        return ok.astype(bool)

    def renderImage(self, type=0):
        """TopFu::renderImage -> uint8 (rows, cols, 4) image (host copy).  type: the reference's
        IVisualisationEngine::RenderImageType (0 shaded greyscale = TopFu::renderImage, 1 greyscale
        from image normals, 2 colour from volume (greyscale for Voxel_s), 3 colour from normal,
        4 colour from confidence)."""
        L.check(L.load().tf_render_image_type(self._h, int(type), None, 0), "tf_render_image_type")
        return self.download(L.TF_BUF_GREY).view(np.uint8).reshape(self.H, self.W, 4)

    def frame_grey(self):
        """The grey image renderImage produced inside the last tracked frame (no re-render)."""
        return self.download(L.TF_BUF_GREY).view(np.uint8).reshape(self.H, self.W, 4)

    def getCameraPose(self):
        rt = np.zeros(12, np.float32)
        L.check(L.load().tf_get_pose(self._h, _ptr(rt)), "tf_get_pose")
        m = np.eye(4, dtype=np.float32)
        m[:3, :4] = rt.reshape(3, 4)
        return m

    def reset(self):
        L.check(L.load().tf_reset(self._h), "tf_reset")

    @property
    def last_stats(self):
        """The counters after the last frame (tf_get_stats: waits for the frame's remaining work --
        a frame call returns once its result is known, with its later stages still running)."""
        return self.stats() if self._framed else None

    def stats(self):
        s = L.TfStats()
        L.check(L.load().tf_get_stats(self._h, ctypes.byref(s)), "tf_get_stats")
        return s.as_dict()

    def totals(self):
        """Frame totals accumulated on the device since creation / reset_totals() (tf_totals)."""
        t = L.TfTotals()
        L.check(L.load().tf_get_totals(self._h, ctypes.byref(t)), "tf_get_totals")
        return t.as_dict()

    def reset_totals(self):
        L.check(L.load().tf_reset_totals(self._h), "tf_reset_totals")

    def stream(self):
        return L.load().tf_get_stream(self._h)

    POSE_ALGEBRAS = {"canonical": 0, "opencv2": 2, "opencv4": 4, "svd": 4}

    def set_pose_algebra(self, algebra):
        """The ICP iterations' det / solve / Rodrigues (tf_set_pose_algebra): the reference's OpenCV
        algebra, "opencv4" (default; = "svd") or "opencv2" (2.4.9), or "canonical" (LU + 2 x 2 block
        Schur solve + sinc Rodrigues: a shorter serial tail, not the reference's arithmetic)."""
        a = self.POSE_ALGEBRAS[algebra] if isinstance(algebra, str) else int(algebra)
        L.check(L.load().tf_set_pose_algebra(self._h, a), "tf_set_pose_algebra")

    def pose_algebra(self):
        v = ctypes.c_int()
        L.check(L.load().tf_get_pose_algebra(self._h, ctypes.byref(v)), "tf_get_pose_algebra")
        return v.value

    def icp_persistent(self):
        """True when ICP runs as one persistent launch per frame."""
        v = ctypes.c_int()
        L.check(L.load().tf_get_schedule(self._h, ctypes.byref(v)), "tf_get_schedule")
        return bool(v.value)

    # -- per-stage HIP-event timing ----------------------------------------------------
    def profile(self, enable=True, stages=None, every=1):
        """Time every stage (enable=True), none, or only the named stages (HIP events on the
        context stream; each timed stage costs GPU time of its own), on every `every`-th frame."""
        if stages is None:
            L.check(L.load().tf_profile_enable(self._h, int(enable)), "tf_profile_enable")
        else:
            mask = 0
            for s in stages:
                mask |= 1 << L.STAGE_NAMES.index(s)
            L.check(L.load().tf_profile_stages(self._h, mask if enable else 0), "tf_profile_stages")
        L.check(L.load().tf_profile_sample(self._h, int(every)), "tf_profile_sample")
        L.check(L.load().tf_profile_reset(self._h), "tf_profile_reset")

    def profile_read(self):
        n = len(L.STAGE_NAMES)
        ms = np.zeros(n, np.float64)
        cnt = np.zeros(n, np.int64)
        L.check(L.load().tf_profile_read(self._h, _ptr(ms), _ptr(cnt), n), "tf_profile_read")
        return {name: (float(ms[i]), int(cnt[i])) for i, name in enumerate(L.STAGE_NAMES)}

    # -- stage entry points (parity tests) ------------------------------------------------
    def stage_preprocess(self, depth):
        """computeDists + bilateral + truncation + pyramid + vertex/normal maps (host depth)."""
        d = np.ascontiguousarray(depth, np.uint16)
        assert d.shape == (self.H, self.W), d.shape
        L.check(L.load().tf_stage_preprocess_host(self._h, _ptr(d), self.W * 2), "tf_stage_preprocess_host")

    def stage_icp(self):
        aff = np.zeros(12, np.float32)
        ok = ctypes.c_int()
        it = ctypes.c_int()
        L.check(L.load().tf_stage_icp(self._h, _ptr(aff), ctypes.byref(ok), ctypes.byref(it)), "tf_stage_icp")
        return bool(ok.value), aff.reshape(3, 4), it.value

    def stage_alloc(self, pose_rt):
        L.check(L.load().tf_stage_alloc(self._h, _ptr(_rt(pose_rt))), "tf_stage_alloc")

    def stage_integrate(self, pose_rt):
        L.check(L.load().tf_stage_integrate(self._h, _ptr(_rt(pose_rt))), "tf_stage_integrate")

    def stage_expected_depths(self, pose_rt):
        L.check(L.load().tf_stage_expected_depths(self._h, _ptr(_rt(pose_rt))), "tf_stage_expected_depths")

    def stage_raycast(self, invM_rt, update_visible):
        L.check(L.load().tf_stage_raycast(self._h, _ptr(_rt(invM_rt)), int(update_visible)), "tf_stage_raycast")

    def stage_icp_maps(self, invM_rt):
        L.check(L.load().tf_stage_icp_maps(self._h, _ptr(_rt(invM_rt))), "tf_stage_icp_maps")

    def stage_render_grey(self, invM_rt):
        L.check(L.load().tf_stage_render_grey(self._h, _ptr(_rt(invM_rt))), "tf_stage_render_grey")
        return self.download(L.TF_BUF_GREY).view(np.uint8).reshape(self.H, self.W, 4)

    def stage_reset_scene(self):
        L.check(L.load().tf_stage_reset_scene(self._h), "tf_stage_reset_scene")

    def stage_swap_pyramids(self):
        L.check(L.load().tf_stage_swap_pyramids(self._h), "tf_stage_swap_pyramids")

    # -- state transfer ------------------------------------------------------------------
    def nbytes(self, which, level=0):
        n = ctypes.c_size_t()
        L.check(L.load().tf_buffer_bytes(self._h, which, level, ctypes.byref(n)), "tf_buffer_bytes")
        return n.value

    def download(self, which, level=0):
        n = self.nbytes(which, level)
        buf = np.empty(n, np.uint8)
        L.check(L.load().tf_download(self._h, which, level, _ptr(buf), n), "tf_download")
        return buf

    def upload(self, which, arr, level=0):
        a = np.ascontiguousarray(arr)
        n = self.nbytes(which, level)
        assert a.nbytes == n, (a.nbytes, n)
        L.check(L.load().tf_upload(self._h, which, level, _ptr(a), n), "tf_upload")

    def set_pose(self, rt):
        L.check(L.load().tf_set_pose(self._h, _ptr(_rt(rt))), "tf_set_pose")

    def time_stage(self, stage, pose_rt, iters):
        """ms per launch of `iters` back-to-back launches of a stage's kernels (HIP events on
        the context stream); stage: "integrate" or "raycast_icp"."""
        ms = ctypes.c_float()
        L.check(L.load().tf_time_stage(self._h, L.STAGE_NAMES.index(stage), _ptr(_rt(pose_rt)), int(iters),
                                       ctypes.byref(ms)), "tf_time_stage")
        return float(ms.value)

    def set_counters(self, lastFreeBlockId, lastFreeExcessListId, noVisibleEntries):
        L.check(L.load().tf_set_counters(self._h, lastFreeBlockId, lastFreeExcessListId, noVisibleEntries),
                "tf_set_counters")

    def fuse_frames(self, dev_frames, poses_w2c, stride=None, pitch=0, intr=None):
        """tf_scene_fuse_frames: computeDists + AllocateSceneFromDepth + IntegrateIntoScene (+ the
        swapping engine) per frame of a device-resident uint16 batch (`dev_frames`: device address
        of frame 0) at the world->camera poses `poses_w2c` (n x 3 x 4 or n x 12); returns the
        per-frame records (numpy structured array, L.FUSE_RECORD_DTYPE)."""
        P = np.ascontiguousarray(np.asarray(poses_w2c, np.float32).reshape(-1, 12))
        n = len(P)
        rec = np.zeros(n, L.FUSE_RECORD_DTYPE)
        if stride is None:
            stride = self.W * self.H * 2
        ip = None if intr is None else _ptr(np.ascontiguousarray(intr, np.float32))
        L.check(L.load().tf_scene_fuse_frames(self._h, ip, ctypes.c_void_p(int(dev_frames)), int(stride), int(pitch),
                                              _ptr(P), n, _ptr(rec)), "tf_scene_fuse_frames")
        return rec

    def alloc_list(self):
        """LocalVBA::allocationList (the free-block stack)."""
        return self.download(L.TF_BUF_ALLOC_LIST).view(np.int32)

    def excess_list(self):
        return self.download(L.TF_BUF_EXCESS_LIST).view(np.int32)

    # swapping (GlobalCache in HBM)
    def swap(self):
        """The swapping engine once (IntegrateGlobalIntoLocal + SaveToGlobalMemory)."""
        L.check(L.load().tf_scene_swap(self._h), "tf_scene_swap")

    def swap_in(self):
        """IntegrateGlobalIntoLocal alone."""
        L.check(L.load().tf_scene_swap_in(self._h), "tf_scene_swap_in")

    def swap_out(self):
        """SaveToGlobalMemory alone."""
        L.check(L.load().tf_scene_swap_out(self._h), "tf_scene_swap_out")

    def swap_counts(self):
        """(swapped in, swapped out, reallocated) blocks of the last frame / call."""
        out = np.zeros(3, np.int32)
        L.check(L.load().tf_swap_counts(self._h, _ptr(out)), "tf_swap_counts")
        return tuple(int(v) for v in out)

    def swap_state(self):
        return self.download(L.TF_BUF_SWAP_STATE)

    def swap_stored_flags(self):
        return self.download(L.TF_BUF_SWAP_STORED_FLAGS)

    def swap_stored(self):
        return self.download(L.TF_BUF_SWAP_STORED).view(VOXEL_DTYPE)

    def swap_save(self, path):
        L.check(L.load().tf_swap_save(self._h, str(path).encode()), "tf_swap_save")

    def swap_load(self, path):
        L.check(L.load().tf_swap_load(self._h, str(path).encode()), "tf_swap_load")

    # -- scene checkpoints (additions: tf_scene_save / tf_scene_load; the reference cannot save its map) ----
    def save_scene(self, path):
        """The state a sequence resumes from -- live hash entries and their blocks, visible list, free
        lists, counters, pose, tracker maps -- as a file sized by what is live (tf_scene_save)."""
        L.check(L.load().tf_scene_save(self._h, str(path).encode()), "tf_scene_save")

    def load_scene(self, path):
        """Replaces this context's scene, pose and frame counter by the file's (tf_scene_load): from here
        on it is the saving context, bit for bit.  Capacities, image size and scene parameters must be the
        file's; a refused file (TfError, TF_INVALID_ARG) leaves the context as it was."""
        L.check(L.load().tf_scene_load(self._h, str(path).encode()), "tf_scene_load")
        self._framed = True

    def scene_ckpt_times(self):
        """What the last save_scene / load_scene spent (tf_scene_ckpt_times): a dict of milliseconds --
        copies, file, check (the record check and checksum), call (host clock), and on a context created with
        TFUSION_CKPT_TIMING=1 index_kernels, block_kernels (HIP events) -- and block_kernel_bytes."""
        ms = np.zeros(8, np.float64)
        L.check(L.load().tf_scene_ckpt_times(self._h, _ptr(ms)), "tf_scene_ckpt_times")
        return dict(zip(("index_kernels", "block_kernels", "copies", "file", "call", "block_kernel_bytes", "check"), ms.tolist()))

    # -- map checkpoints (additions: tf_map_save / tf_map_load): a swapping context's too, both tiers ----
    def save_map(self, path):
        """save_scene's file on a context without swapping; on a swapping context the version-2 file,
        which adds the GlobalCache: swap states, stored flags and the stored blocks (tf_map_save)."""
        L.check(L.load().tf_map_save(self._h, str(path).encode()), "tf_map_save")

    def load_map(self, path):
        """load_scene for either kind of context (tf_map_load): the file's use_swapping must be the
        context's.  A refused file leaves the context, GlobalCache included, as it was."""
        L.check(L.load().tf_map_load(self._h, str(path).encode()), "tf_map_load")
        self._framed = True

    def load_map_resized(self, path):
        """load_map into a context whose n_buckets, n_excess or n_blocks are not the file's (tf_map_load_resized):
        the records are re-hashed on the way in, as if inserted one by one into a reset table; records without
        a block position are dropped.  Returns the report as a dict (records_carried, records_dropped, blocks,
        cache_blocks, excess_used, longest_chain).  A map that does not fit is TfError with TF_CAPACITY; its
        .report holds what would have been needed, and the context is as it was."""
        rep = L.TfResizeReport()
        status = L.load().tf_map_load_resized(self._h, str(path).encode(), ctypes.byref(rep))
        if status != L.TF_OK:
            err = L.TfError(status, "tf_map_load_resized")
            err.report = rep.as_dict() if status == L.TF_CAPACITY else None
            raise err
        self._framed = True
        return rep.as_dict()

    def merge_map(self, path, block_offset=(0, 0, 0)):
        """Fuses a version-1 checkpoint into the live scene (tf_map_merge): the file's records with a block, moved by
        block_offset whole blocks, are combined voxel by voxel where the scene already holds the position and
        inserted where it does not; pose, visible list and tracker maps stay.  Returns the report as a dict
        (records_combined, records_inserted, records_revived, records_skipped, blocks_used, excess_used).  A file
        that does not fit the free lists is TfError with TF_CAPACITY; its .report holds what would have been
        needed.  Every refusal leaves the context as it was."""
        rep = L.TfMergeReport()
        off = (ctypes.c_int * 3)(*(int(v) for v in block_offset))
        status = L.load().tf_map_merge(self._h, str(path).encode(), off, ctypes.byref(rep))
        if status != L.TF_OK:
            err = L.TfError(status, "tf_map_merge")
            err.report = rep.as_dict() if status == L.TF_CAPACITY else None
            raise err
        return rep.as_dict()

    @classmethod
    def from_map(cls, path, device=None, resize=False, **overrides):
        """from_scene for a map checkpoint of either version: the context is built from the file's
        params, swapping included.  resize=True: `overrides` may change n_buckets, n_excess and n_blocks,
        and the file is loaded with load_map_resized (the report is kept as .resize_report)."""
        return cls._from_file(path, device, overrides, L.map_file_info, "_load_map_resized_keep" if resize else "load_map")

    def _load_map_resized_keep(self, path):
        self.resize_report = self.load_map_resized(path)

    @classmethod
    def from_scene(cls, path, device=None, **overrides):
        """A context built from the file's params (with `overrides` applied, as default_params takes
        them) that has loaded the file; the pose algebra is the file's too."""
        return cls._from_file(path, device, overrides, L.scene_file_info, "load_scene")

    @classmethod
    def _from_file(cls, path, device, overrides, file_info, load):
        info = file_info(path)
        p = info["params"]
        for k, v in overrides.items():
            if k == "icp_iter_num":
                for i in range(4):
                    p.icp_iter_num[i] = int(v[i]) if i < len(v) else 0
            elif k in ("rgb_intr", "depth_to_rgb"):
                arr = getattr(p, k)
                for i, x in enumerate(v):
                    arr[i] = float(x)
            else:
                setattr(p, k, v)
        t = cls(p, device=device)
        try:
            t.set_pose_algebra(info["pose_algebra"])
            getattr(t, load)(path)
        except Exception:
            t.close()
            raise
        return t

    # -- mesh extraction (additions: tf_mesh_*; the reference has no mesher) ------------------------
    # whole=True: the reading over both tiers of a swapping scene (tf_mesh_extract_whole, TF_MESH_WHOLE) -- every
    # entry with voxel data in the VBA or the GlobalCache, stored blocks read where they lie, pending merges
    # combined on the fly; without stored data it is the resident mesh byte for byte.  No colours, not indexed.
    def mesh_count(self, whole=False):
        """Triangles the scene's mesh has (the count pass alone)."""
        n = ctypes.c_longlong()
        if whole:
            L.check(L.load().tf_mesh_extract_whole(self._h, None, None, 0, ctypes.byref(n)), "tf_mesh_extract_whole")
        else:
            L.check(L.load().tf_mesh_extract(self._h, None, 0, ctypes.byref(n)), "tf_mesh_extract")
        return n.value

    def mesh(self, whole=False):
        """The scene's surface as (n, 3, 3) float32 triangles -- marching tetrahedra over the voxel
        block hash, in the fixed order of tf_mesh_extract, right-hand normals towards free space.
        Counts, allocates a device buffer through the library's HIP runtime, extracts, downloads."""
        n = self.mesh_count(whole)
        out = np.empty((n, 3, 3), np.float32)
        if n == 0:
            return out
        hip = L.hip_runtime()
        dev = ctypes.c_void_p()
        if hip.hipMalloc(ctypes.byref(dev), ctypes.c_size_t(out.nbytes)) != 0:
            raise L.TfError(L.TF_OOM, "hipMalloc (mesh)")
        try:
            m = ctypes.c_longlong()
            if whole:
                L.check(L.load().tf_mesh_extract_whole(self._h, dev, None, n, ctypes.byref(m)), "tf_mesh_extract_whole")
            else:
                L.check(L.load().tf_mesh_extract(self._h, dev, n, ctypes.byref(m)), "tf_mesh_extract")
            assert m.value == n, (m.value, n)
            if hip.hipMemcpy(_ptr(out), dev, ctypes.c_size_t(out.nbytes), 2) != 0:      # hipMemcpyDeviceToHost
                raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (mesh)")
        finally:
            hip.hipFree(dev)
        return out

    def mesh_attr(self, normals=True, colours=False, whole=False):
        """mesh() with per-vertex attributes (tf_mesh_extract_attr): (triangles (n, 3, 3) float32,
        normals (n, 3, 3) float32 or None, colours (n, 3, 4) uint8 RGBA or None), the same triangles
        in the same order.  Normals are the normalised TSDF gradient (towards free space), colours
        come from the colour plane (voxel_rgb contexts only; never with whole=True)."""
        if whole and colours:
            raise L.TfError(L.TF_INVALID_ARG, "mesh_attr (whole with colours)")
        n = self.mesh_count(whole)
        outs = [np.empty((n, 3, 3), np.float32), np.empty((n, 3, 3), np.float32) if normals else None,
                np.empty((n, 3, 4), np.uint8) if colours else None]
        if n == 0 and not (colours and not self.params_.voxel_rgb):     # (that one is the library's TF_INVALID_ARG)
            return tuple(outs)
        hip = L.hip_runtime()
        devs = []
        try:
            for o in outs:
                d = ctypes.c_void_p()
                if o is not None and hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(o.nbytes, 16))) != 0:
                    raise L.TfError(L.TF_OOM, "hipMalloc (mesh)")
                devs.append(d)
            m = ctypes.c_longlong()
            if whole:
                L.check(L.load().tf_mesh_extract_whole(self._h, devs[0], devs[1], n, ctypes.byref(m)), "tf_mesh_extract_whole")
            else:
                L.check(L.load().tf_mesh_extract_attr(self._h, devs[0], devs[1], devs[2], n, ctypes.byref(m)), "tf_mesh_extract_attr")
            assert m.value == n, (m.value, n)
            for o, d in zip(outs, devs):
                if o is not None and n and hip.hipMemcpy(_ptr(o), d, ctypes.c_size_t(o.nbytes), 2) != 0:   # hipMemcpyDeviceToHost
                    raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (mesh)")
        finally:
            for d in devs:
                if d:
                    hip.hipFree(d)
        return tuple(outs)

    def mesh_indexed_count(self):
        """(vertices, triangles) the scene's indexed mesh has (the count passes alone)."""
        nv, nt = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(L.load().tf_mesh_extract_indexed(self._h, None, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)),
                "tf_mesh_extract_indexed")
        return nv.value, nt.value

    def mesh_indexed(self, normals=False, colours=False):
        """mesh() with shared vertices (tf_mesh_extract_indexed): (vertices (nv, 3) float32, indices (nt, 3)
        uint32, normals (nv, 3) float32 or None, colours (nv, 4) uint8 RGBA or None).  vertices[indices] is
        mesh() bit for bit, normals[indices] / colours[indices] are mesh_attr()'s.  A vertex is the cube edge it
        lies on: edges are never merged, even where their positions coincide."""
        if colours and not self.params_.voxel_rgb:
            raise L.TfError(L.TF_INVALID_ARG, "mesh_indexed (colours without voxel_rgb)")
        nv, nt = self.mesh_indexed_count()
        outs = [np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32) if normals else None,
                np.empty((nv, 4), np.uint8) if colours else None, np.empty((nt, 3), np.uint32)]
        if nt == 0:
            return outs[0], outs[3], outs[1], outs[2]
        hip = L.hip_runtime()
        devs = []
        try:
            for o in outs:
                d = ctypes.c_void_p()
                if o is not None and hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(o.nbytes, 16))) != 0:
                    raise L.TfError(L.TF_OOM, "hipMalloc (mesh)")
                devs.append(d)
            mv, mt = ctypes.c_longlong(), ctypes.c_longlong()
            L.check(L.load().tf_mesh_extract_indexed(self._h, devs[0], devs[1], devs[2], nv, devs[3], nt, ctypes.byref(mv),
                                                     ctypes.byref(mt)), "tf_mesh_extract_indexed")
            assert (mv.value, mt.value) == (nv, nt), (mv.value, mt.value, nv, nt)
            for o, d in zip(outs, devs):
                if o is not None and hip.hipMemcpy(_ptr(o), d, ctypes.c_size_t(o.nbytes), 2) != 0:   # hipMemcpyDeviceToHost
                    raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (mesh)")
        finally:
            for d in devs:
                if d:
                    hip.hipFree(d)
        return outs[0], outs[3], outs[1], outs[2]

    # the whole reading with shared vertices (tf_mesh_extract_indexed_whole): the edge bits keyed by a compact
    # numbering of the entries that resolve, so blocks in the GlobalCache own vertices too
    def mesh_indexed_whole_count(self):
        """(vertices, triangles) the whole map's indexed mesh has (the count passes alone)."""
        nv, nt = ctypes.c_longlong(), ctypes.c_longlong()
        L.check(L.load().tf_mesh_extract_indexed_whole(self._h, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)),
                "tf_mesh_extract_indexed_whole")
        return nv.value, nt.value

    def mesh_indexed_whole(self, normals=False):
        """mesh(whole=True) with shared vertices: (vertices (nv, 3) float32, indices (nt, 3) uint32, normals
        (nv, 3) float32 or None).  vertices[indices] is mesh(whole=True) bit for bit, normals[indices] are
        mesh_attr(whole=True)'s.  Without stored data it is mesh_indexed() byte for byte."""
        nv, nt = self.mesh_indexed_whole_count()
        outs = [np.empty((nv, 3), np.float32), np.empty((nv, 3), np.float32) if normals else None, np.empty((nt, 3), np.uint32)]
        if nt == 0:
            return outs[0], outs[2], outs[1]
        hip = L.hip_runtime()
        devs = []
        try:
            for o in outs:
                d = ctypes.c_void_p()
                if o is not None and hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(o.nbytes, 16))) != 0:
                    raise L.TfError(L.TF_OOM, "hipMalloc (mesh)")
                devs.append(d)
            mv, mt = ctypes.c_longlong(), ctypes.c_longlong()
            L.check(L.load().tf_mesh_extract_indexed_whole(self._h, devs[0], devs[1], nv, devs[2], nt, ctypes.byref(mv),
                                                           ctypes.byref(mt)), "tf_mesh_extract_indexed_whole")
            assert (mv.value, mt.value) == (nv, nt), (mv.value, mt.value, nv, nt)
            for o, d in zip(outs, devs):
                if o is not None and hip.hipMemcpy(_ptr(o), d, ctypes.c_size_t(o.nbytes), 2) != 0:   # hipMemcpyDeviceToHost
                    raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (mesh)")
        finally:
            for d in devs:
                if d:
                    hip.hipFree(d)
        return outs[0], outs[2], outs[1]

    def save_mesh_indexed_whole(self, path, normals=False):
        """The whole map's indexed mesh as a binary PLY (tf_mesh_save_ply_indexed_whole): no host weld, and
        written in bounded pieces -- the host holds one chunk (TFUSION_MESH_CHUNK_BYTES), whatever the map."""
        L.check(L.load().tf_mesh_save_ply_indexed_whole(self._h, str(path).encode(), L.TF_MESH_NORMALS if normals else 0),
                "tf_mesh_save_ply_indexed_whole")

    def save_mesh(self, path, normals=False, colours=False, indexed=False, whole=False):
        """The mesh as a binary PLY with welded vertices (tf_mesh_save_ply); with normals / colours,
        nx ny nz / red green blue alpha per vertex (tf_mesh_save_ply_attr).  indexed: the vertex table of
        mesh_indexed() as it is, no host weld (tf_mesh_save_ply_indexed).  whole: the whole map's mesh through
        the same writer (one download, one weld: the caller's memory bounds it); not with indexed or colours."""
        attrs = (L.TF_MESH_NORMALS if normals else 0) | (L.TF_MESH_COLOURS if colours else 0) | (L.TF_MESH_WHOLE if whole else 0)
        if indexed:
            L.check(L.load().tf_mesh_save_ply_indexed(self._h, str(path).encode(), attrs), "tf_mesh_save_ply_indexed")
            return
        if not normals and not colours and not whole:
            L.check(L.load().tf_mesh_save_ply(self._h, str(path).encode()), "tf_mesh_save_ply")
            return
        L.check(L.load().tf_mesh_save_ply_attr(self._h, str(path).encode(), attrs), "tf_mesh_save_ply_attr")

    # -- scene queries (additions: tf_scene_query / tf_scene_slice; DESIGN.md §5 Scene queries) --------------
    _QUERY_OUTS = (("sdf_nearest", np.float32, ()), ("entry", np.int32, ()), ("sdf", np.float32, ()),
                   ("confidence", np.float32, ()), ("normal", np.float32, (3,)), ("colour", np.uint8, (4,)))

    def _query(self, n, normals, colours, call, where):
        want = [k for k, _, _ in self._QUERY_OUTS if (k != "normal" or normals) and (k != "colour" or colours)]
        outs = {k: np.empty((n,) + tail, dt) for k, dt, tail in self._QUERY_OUTS if k in want}
        hip = L.hip_runtime()
        qo = L.TfQueryOut()
        devs = []
        try:
            for k, o in outs.items():
                d = ctypes.c_void_p()
                if hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(o.nbytes, 16))) != 0:
                    raise L.TfError(L.TF_OOM, "hipMalloc (query)")
                devs.append(d)
                setattr(qo, k, d.value)
            L.check(call(hip, qo, devs), where)
            for o, d in zip(outs.values(), devs):
                if n and hip.hipMemcpy(_ptr(o), d, ctypes.c_size_t(o.nbytes), 2) != 0:      # hipMemcpyDeviceToHost
                    raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (query)")
        finally:
            for d in devs:
                if d:
                    hip.hipFree(d)
        return outs

    @staticmethod
    def _query_units(units):
        if units not in ("m", "voxels"):
            raise L.TfError(L.TF_INVALID_ARG, f"query units {units!r} (\"m\" or \"voxels\")")
        return L.TF_QUERY_METRES if units == "m" else L.TF_QUERY_VOXELS

    def query(self, points, units="m", whole=False, normals=False, colours=False):
        """The TSDF at host points (n, 3) float32, in metres or ("voxels") voxel units (tf_scene_query): a dict of
        numpy arrays -- sdf_nearest, entry, sdf, confidence, and with normals / colours normal (n, 3) (the SDF
        gradient as the reference leaves it) / colour (n, 4) RGBA (voxel_rgb contexts, never with whole=True).
        A point outside +-262136 voxels reads as nothing (1, -1, 1, 0, zeros).  whole: both tiers of a swapping
        scene.  Through temporary device buffers."""
        pts = np.ascontiguousarray(points, np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3:
            raise L.TfError(L.TF_INVALID_ARG, "query points: (n, 3) float32")
        n, u, r = len(pts), self._query_units(units), L.TF_VIEW_WHOLE if whole else L.TF_VIEW_RESIDENT

        def call(hip, qo, devs):
            d = ctypes.c_void_p()
            if hip.hipMalloc(ctypes.byref(d), ctypes.c_size_t(max(pts.nbytes, 16))) != 0:
                raise L.TfError(L.TF_OOM, "hipMalloc (query)")
            devs.append(d)
            if n and hip.hipMemcpy(d, _ptr(pts), ctypes.c_size_t(pts.nbytes), 1) != 0:      # hipMemcpyHostToDevice
                raise L.TfError(L.TF_HIP_ERROR, "hipMemcpy (query)")
            return L.load().tf_scene_query(self._h, d, n, u, r, ctypes.byref(qo))
        return self._query(n, normals, colours, call, "tf_scene_query")

    def slice(self, origin, u, v, cols, rows, units="m", whole=False, normals=False, colours=False):
        """query() on the plane origin + x * u + y * v, x < cols, y < rows (tf_scene_slice; the points are made on
        the device, in float32): the same dict with arrays of shape (rows, cols[, k])."""
        o3, u3, v3 = (np.ascontiguousarray(a, np.float32).reshape(3) for a in (origin, u, v))
        cols, rows = int(cols), int(rows)
        if cols <= 0 or rows <= 0:
            raise L.TfError(L.TF_INVALID_ARG, "slice size")
        un, r = self._query_units(units), L.TF_VIEW_WHOLE if whole else L.TF_VIEW_RESIDENT

        def call(hip, qo, devs):
            return L.load().tf_scene_slice(self._h, _ptr(o3), _ptr(u3), _ptr(v3), cols, rows, un, r, ctypes.byref(qo))
        outs = self._query(cols * rows, normals, colours, call, "tf_scene_slice")
        return {k: a.reshape((rows, cols) + a.shape[1:]) for k, a in outs.items()}

    # typed views
    def hash(self):
        return self.download(L.TF_BUF_HASH).view(HASH_DTYPE)

    def vba(self):
        return self.download(L.TF_BUF_VBA).view(VOXEL_DTYPE)

    def vba_rgb(self):
        """voxel_rgb: the colour plane, uint32 per voxel (r | g << 8 | b << 16 | w_color << 24)."""
        return self.download(L.TF_BUF_VBA_RGB).view(np.uint32)

    def visible_ids(self):
        n = self.stats()["noVisibleEntries"]
        return self.download(L.TF_BUF_VISIBLE_IDS).view(np.int32)[:n]

    def visible_type(self):
        return self.download(L.TF_BUF_VISIBLE_TYPE)

    def range_image(self):
        return self.download(L.TF_BUF_RANGE).view(np.float32).reshape(self.H, self.W, 2)

    def raycast_result(self):
        return self.download(L.TF_BUF_RAYCAST).view(np.float32).reshape(self.H, self.W, 4)

    def dists(self):
        return self.download(L.TF_BUF_DISTS).view(np.float32).reshape(self.H, self.W)

    def level_shape(self, l):
        return self.H >> l, self.W >> l

    def curr_depth(self, l):
        return self.download(L.TF_BUF_DEPTH, l).view(np.uint16).reshape(self.level_shape(l))

    def curr_maps(self, l):
        h, w = self.level_shape(l)
        return (self.download(L.TF_BUF_CURR_POINTS, l).view(np.float32).reshape(h, w, 4),
                self.download(L.TF_BUF_CURR_NORMALS, l).view(np.float32).reshape(h, w, 4))

    def prev_maps(self, l):
        h, w = self.level_shape(l)
        return (self.download(L.TF_BUF_PREV_POINTS, l).view(np.float32).reshape(h, w, 4),
                self.download(L.TF_BUF_PREV_NORMALS, l).view(np.float32).reshape(h, w, 4))
