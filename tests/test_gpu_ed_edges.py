"""CreateExpectedDepths on constructed lists (tests/ed_cases.py) against the oracle's expected_depths, bit for bit over
the whole range buffer -- W x H x 2 floats, the area outside the /8 region included -- plus noTotalBlocks.  No
tolerances.  The lists put boxes on the index edges of the projection's binning (tf_ed.h) and of the fill
(ed_fill_block, ed_tile_range in tf_render.hip): rows and columns past the /8 region, the below bins, the segment
queue's overflow, visible counts around a chunk and around TFUSION_ED_LDS_MAX_N, caps that land on a block, a chunk
boundary and the last entry; tests/test_ed_cases.py asserts on the CPU that each list holds what it is for.

  a  test_stage, test_stage_caps        k_ed_project + k_ed_fill through stage_expected_depths, both fill paths
  b  test_spill_chain                   one context through a chain of lists: the fill's spill record against a memset
  c  test_engine_entry, test_free_view  tf_vis_expected_depths; a free view's scan + expected_depths, both readings
  d  test_frame_path                    the projection inside k_integrate, the fill and the tiles' bin ranges inside
                                        k_raycast_pair, on a sequence with near and wide blocks injected before frame 2

What mutations of the kernels these catch: profiles/ed_edges_mutation_check.txt."""
import numpy as np
import pytest

import ed_cases as E
import view_ref as V
from parity_util import DeviceFrames, assert_bit_exact
from test_ed_cases import boxes, expected

pytestmark = pytest.mark.gpu

ENVS = ("unset", str(E.LDS_MAX_N), "0")
RECOGNISABLE = np.float32(123.25)


def _create(env, **params):
    """A TopFu created under TFUSION_ED_LDS_MAX_N = env (read by tf_create)."""
    from topfusion_amd import TopFu, default_params
    with pytest.MonkeyPatch.context() as mp:
        if env == "unset":
            mp.delenv("TFUSION_ED_LDS_MAX_N", raising=False)
        else:
            mp.setenv("TFUSION_ED_LDS_MAX_N", env)
        return TopFu(default_params(**params))


class Side:
    """A GPU context and an oracle of one size, with one of the constructed scenes in both."""

    def __init__(self, O, W, H, env, **over):
        from topfusion_amd import _lib
        self.L, self.O, self.W, self.H = _lib, O, W, H
        self.g = _create(env, **E.params_kw(W, H, **over))
        self.o = O.Oracle(O.default_params(**E.params_kw(W, H, **over)))
        self.s = None

    def load(self, s, hash=None):
        if self.s is not s or hash is not None:
            h = s.hash if hash is None else hash
            self.g.upload(self.L.TF_BUF_HASH, h)
            self.o.upload_hash(h)
            self.s = s if hash is None else None
        return self

    def put_list(self, s, ids):
        buf = np.zeros(E.TABLES["vis_capacity"], np.int32)
        buf[:len(ids)] = ids
        self.g.upload(self.L.TF_BUF_VISIBLE_IDS, buf)
        self.g.set_counters(*s.counters(len(ids)))
        self.o.upload_visible_ids(ids)
        self.o.set_counters(*s.counters(len(ids)))

    def compare(self, tag):
        assert_bit_exact(f"{tag}: range image", self.g.range_image(), self.o.range_image())
        got, want = self.g.stats()["noTotalBlocks"], self.o.counters()["noTotalBlocks"]
        assert got == want, f"{tag}: noTotalBlocks gpu {got} oracle {want}"

    def run(self, tag, s, ids, pose, engine=False):
        """CreateExpectedDepths of a list on both sides, through the stage or the engine entry point."""
        self.put_list(s, ids)
        if engine:
            from test_gpu_engines import _f, _ok
            _ok(self.L.load().tf_vis_expected_depths(self.g._h, _f(s.intr), _f(pose)), "tf_vis_expected_depths")
        else:
            self.g.stage_expected_depths(pose)
        self.o.expected_depths(pose)
        self.compare(tag)

    def close(self):
        self.g.close()


@pytest.fixture(scope="module")
def sides(oracle_mod):
    """Contexts shared per (size, TFUSION_ED_LDS_MAX_N)."""
    made = {}

    def get(W, H, env):
        if (W, H, env) not in made:
            made[(W, H, env)] = Side(oracle_mod, W, H, env)
        return made[(W, H, env)]

    yield get
    for side in made.values():
        side.close()


def _size_id(p):
    return f"{p[0]}x{p[1]}"


# ---- a. the stand-alone stage ----------------------------------------------------------------------------
STAGE_CASES = ([(size, fam) for size in E.BIG_SIZES for fam in E.FAMILIES + E.COUNT_FAMILIES]
               + [(size, fam) for size in E.SMALL_SIZES for fam in ("far", "near", "straddle")])


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("pose_name", sorted(E.POSES))
@pytest.mark.parametrize("size,fam", STAGE_CASES, ids=lambda v: _size_id(v) if isinstance(v, tuple) else v)
def test_stage(sides, size, fam, pose_name, env):
    """Every family in its three orders.  Under TFUSION_ED_LDS_MAX_N=512 the count lists run the LDS path at 511 and
    512 entries and the atomic path at 513; under 0 everything runs the atomic path."""
    s = E.scene(*size)
    side = sides(*size, env).load(s)
    for order in E.ORDERS:
        side.run(f"{_size_id(size)} {pose_name} {fam} {order} [{env}]", s, s.ordered(pose_name, fam, order), E.POSES[pose_name])


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("order", E.ORDERS)
@pytest.mark.parametrize("pose_name", sorted(E.POSES))
@pytest.mark.parametrize("size", E.BIG_SIZES, ids=_size_id)
def test_stage_caps(oracle_mod, sides, size, pose_name, order, env):
    """max_render_blocks on each edge of cap_points for the list in this order: a context per cap (the cap is a
    creation parameter), the boxes' tile counts from the shared context's oracle."""
    s = E.scene(*size)
    ids = s.ordered(pose_name, "cap", order)
    b = boxes(sides(*size, env).load(s).o, s, ids, pose_name)
    need = b["need"]
    caps = E.cap_points(need, b["box"], b["z"], *size)
    for cap in sorted({caps[k] for k in E.CAP_NAMES}):
        names = "/".join(k for k in E.CAP_NAMES if caps[k] == cap)
        side = Side(oracle_mod, *size, env, max_render_blocks=cap).load(s)
        try:
            side.run(f"{_size_id(size)} {pose_name} cap {names} = {cap} {order} [{env}]", s, ids, E.POSES[pose_name])
            assert side.o.counters()["noTotalBlocks"] == min(cap, int(need.sum()))
        finally:
            side.close()


# ---- b. the spill bookkeeping ----------------------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("size", E.BIG_SIZES, ids=_size_id)
def test_spill_chain(oracle_mod, size, env):
    """One context, never re-created, through lists that write outside the /8 region and lists that do not, across
    both fill paths and a host upload: the oracle memsets the buffer every time, the kernel clears only what its
    previous fill recorded.  (Under 512 the fourth call is the atomic path with its whole-buffer record, the fifth is
    back on the LDS rows.)"""
    s = E.scene(*size)
    side = Side(oracle_mod, *size, env).load(s)
    I, T = E.POSES["identity"], E.POSES["tilted"]
    near, far = s.fam[("identity", "near")], s.fam[("identity", "far")]
    try:
        side.run("1 near", s, near, I)
        side.run("2 far", s, far, I)
        side.run("3 n = 0", s, near[:0], I)
        side.run("4 near at n = 513", s, np.resize(near, E.LDS_MAX_N + 1), I)
        side.run("5 far at n = 300", s, np.resize(far, 300), I)
        filled = np.full((s.H, s.W, 2), RECOGNISABLE, np.float32)
        side.g.upload(side.L.TF_BUF_RANGE, filled)
        side.o.upload_range_image(filled)
        assert_bit_exact("6 uploaded range image", side.g.range_image(), filled)
        side.run("7 far", s, far, I)
        side.run("8 near at the second pose", s, s.fam[("tilted", "near")], T)
        side.run("9 far", s, far, I)
        # + a list that writes past the /8 columns and under the /8 rows but nothing below the LDS rows, so that only
        # the rows' own records say how far down the next clear must reach; then nothing
        b = boxes(side.o, s, far, "identity")
        shallow = far[b["valid"] & ~b["below"]]
        assert (b["past_rc"] & ~b["below"]).any() and (b["under_rr"] & ~b["below"]).any()
        side.run("10 far without the boxes that reach below the LDS rows", s, shallow, I)
        side.run("11 n = 0", s, near[:0], I)
    finally:
        side.close()


# ---- c. the engine and view entry points -----------------------------------------------------------------
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("pose_name", sorted(E.POSES))
@pytest.mark.parametrize("fam", ("near", "straddle", "wide"))
@pytest.mark.parametrize("size", E.BIG_SIZES, ids=_size_id)
def test_engine_entry(sides, size, fam, pose_name, env):
    """tf_vis_expected_depths (the caller's intrinsics and pose)."""
    s = E.scene(*size)
    side = sides(*size, env).load(s)
    for order in E.ORDERS:
        side.run(f"engine {_size_id(size)} {pose_name} {fam} {order} [{env}]", s, s.ordered(pose_name, fam, order),
                 E.POSES[pose_name], engine=True)


VIEW_SCENES = ((64, 48, None), (200, 40, 200))
VIEW_CONTEXT = (36, 28)


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("pose_name", sorted(E.POSES))
@pytest.mark.parametrize("fam", ("near", "straddle", "wide"))
@pytest.mark.parametrize("view", VIEW_SCENES, ids=_size_id)
def test_free_view(oracle_mod, sides, view, fam, pose_name, env):
    """A 64x48 and a 200x40 view of a 36x28 context whose table holds one family: the list is what the view's scan
    finds, in ascending entry order (tests/view_ref.py), the image the oracle's at the view's size and intrinsics; the
    resident and the whole reading give the same bytes on a context without swapping."""
    s = E.scene(*view)
    side = sides(*VIEW_CONTEXT, "unset")
    table = s.hash_only(s.fam[(pose_name, fam)])
    side.load(s, hash=table)
    side.g.set_counters(*s.counters(0))
    pose = E.POSES[pose_name]
    ov = oracle_mod.Oracle(oracle_mod.default_params(**E.params_kw(s.W, s.H, s.intr)))
    lst = V.visible_list(ov, table, pose)
    want, want_total = expected(ov, s, lst, pose, hash=table)
    tag = f"view {_size_id(view)} {pose_name} {fam} [{env}]"
    got = []
    with pytest.MonkeyPatch.context() as mp:
        if env == "unset":
            mp.delenv("TFUSION_ED_LDS_MAX_N", raising=False)
        else:
            mp.setenv("TFUSION_ED_LDS_MAX_N", env)
        for whole in (False, True):
            with side.g.view(s.W, s.H, whole=whole) as v:
                n = v.find_visible(pose, s.intr)
                assert n == len(lst), (tag, whole, n, len(lst))
                assert_bit_exact(f"{tag} whole={whole}: visible list", v.visible_ids(), lst)
                v.expected_depths(pose, s.intr)
                got.append(v.range_image())
                assert_bit_exact(f"{tag} whole={whole}: range image", got[-1], want)
                assert v.stats() == dict(noVisibleEntries=len(lst), noTotalBlocks=want_total), (tag, whole, v.stats())
    assert got[0].tobytes() == got[1].tobytes()


# ---- d. the fused frame path -----------------------------------------------------------------------------
def _frame_pair(O, env, **kw):
    """Both sides after frames 0 and 1 of the sequence with the blocks of ed_cases.frame_setup injected:
    (gpu, oracle, injected entries).  env: "unset", "0", or "mid" -- the threshold between the visible counts before
    and after the injection, with which frame 2 is the first on the fill's atomic path and its CreateICPMaps tiles wait
    for the fill's rows."""
    from topfusion_amd import _lib as L
    from test_gpu_parity import _compare_frame_state
    o, state, entries = E.frame_setup(O, **kw)
    n1 = o.counters()["noVisibleEntries"]
    g = _create(str(E.frame_threshold(n1, len(entries))) if env == "mid" else env, **E.frame_params(**kw))
    seq = E.frame_sequence()
    for k in range(2):
        assert g(seq[k]), f"frame {k}"
    _compare_frame_state(g, o, "frame 1")
    E.frame_load(o, state)
    g.upload(L.TF_BUF_HASH, state["hash"])
    g.upload(L.TF_BUF_VISIBLE_IDS, state["visible_ids"])
    g.set_counters(*state["counters"])
    new = g.vba().reshape(-1, 512)[state["hash"]["ptr"][entries]]
    assert (new["sdf"] == 32767).all() and (new["w"] == 0).all()           # the new blocks' voxels: cleared on the GPU too
    assert_bit_exact("free list", g.alloc_list(), state["alloc_list"])
    return g, o, entries


def _frame_compare(g, o, tag, stats=None):
    from test_gpu_parity import _compare_frame_state
    _compare_frame_state(g, o, tag)
    got, want = (stats or g.stats())["noTotalBlocks"], o.counters()["noTotalBlocks"]
    assert got == want, f"{tag}: noTotalBlocks gpu {got} oracle {want}"


FRAME_CASES = [("unset", False), ("0", False), ("mid", False), ("unset", True)]


@pytest.mark.parametrize("batch", [False, True], ids=["per_call", "batch"])
@pytest.mark.parametrize("env,capped", FRAME_CASES, ids=lambda v: v if isinstance(v, str) else ("capped" if v else "plain"))
def test_frame_path(oracle_mod, env, capped, batch):
    """Frames 2 and 3 through TopFu.__call__, or as one process_frames batch, after the injection; everything
    test_gpu_parity's _run_sequence compares.  capped: a context without ICP iterations whose max_render_blocks frame
    2's list meets exactly at an injected entry that alone decides range pixels the CreateICPMaps rays read
    (ed_cases.frame_cap): the tiles' bin ranges and the fill must keep it, and drop what follows."""
    from test_gpu_parity import compare_scene
    kw = dict(max_render_blocks=E.frame_cap()[0], **E.STILL) if capped else {}
    g, o, entries = _frame_pair(oracle_mod, env, **kw)
    seq = E.frame_sequence()
    dev = None
    try:
        if batch:
            dev = DeviceFrames(seq[2:4])
            okg = g.process_frames(dev.ptr, 2)
            oko = np.array([o(seq[2]), o(seq[3])])
            assert np.array_equal(okg, oko) and oko.all(), (okg, oko)
            _frame_compare(g, o, "batch frames 2..3")
        else:
            for k in (2, 3):
                okg, oko = g(seq[k]), o(seq[k])
                assert okg and oko, f"frame {k}: ok gpu {okg} oracle {oko}"
                _frame_compare(g, o, f"frame {k}", g.last_stats)
                if k == 2 and not capped:
                    assert np.isin(entries, g.visible_ids()).all()
        compare_scene(g, o, "final")
    finally:
        g.close()
        if dev is not None:
            dev.free()
