"""The inputs of tests/test_gpu_ed_edges.py do what they are for -- asserted on the oracle alone (its
ProjectSingleBlock and CreateExpectedDepths, which the stage pin holds to the reference's own code), so that an edit
to tests/ed_cases.py cannot hollow the GPU tests out: per family the boxes of each kind it is built for, the wide
row's queue overflow, the entries each cap drops, the pixels written outside the /8 region and below the LDS rows, the
input condition, and the frame-path injection's conditions."""
import numpy as np
import pytest

import ed_cases as E
import view_ref as V
from parity_util import assert_bit_exact

SCENES = [(W, H, None) for W, H in E.BIG_SIZES + E.SMALL_SIZES] + [(200, 40, 200)]
VIEWS = ((64, 48, None), (200, 40, 200))          # the free views of test_gpu_ed_edges (the second on view_ref's intrinsics)


def oracle_of(O, s, **over):
    o = O.Oracle(O.default_params(**E.params_kw(s.W, s.H, s.intr, **over)))
    o.upload_hash(s.hash)
    return o


def expected(o, s, ids, pose, hash=None):
    """CreateExpectedDepths of a list in the oracle: (whole range image, noTotalBlocks)."""
    if hash is not None:
        o.upload_hash(hash)
    o.upload_visible_ids(ids)
    o.set_counters(*s.counters(len(ids)))
    o.upload_range_image(np.full((s.H, s.W, 2), -7.0, np.float32))       # (CreateExpectedDepths memsets it all)
    o.expected_depths(pose)
    return o.range_image(), o.counters()["noTotalBlocks"]


def boxes(o, s, ids, pose_name):
    """The oracle's projection of a list, with the kinds the kernels branch on."""
    valid, box, z = o.project_blocks(E.POSES[pose_name], ids)
    valid, box = valid.astype(bool), box.astype(np.int64)
    rc, rr, nrows = E.region(s.W, s.H)
    w, h = box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1
    below = valid & (box[:, 3] >= nrows)
    seg = w * (box[:, 3] - np.maximum(box[:, 1], nrows) + 1)
    return dict(valid=valid, box=box, z=z, w=w, h=h, need=np.where(valid, -(-w // E.RB) * -(-h // E.RB), 0),
                past_rc=valid & (box[:, 2] >= rc), under_rr=valid & (box[:, 3] >= rr), below=below,
                below_thread=below & (seg <= E.BELOW_BY_THREAD), below_queued=below & (seg > E.BELOW_BY_THREAD),
                clamp_w=valid & (box[:, 2] == s.W - 1), clamp_h=valid & (box[:, 3] == s.H - 1))


@pytest.fixture(scope="module", params=SCENES, ids=lambda p: f"{p[0]}x{p[1]}")
def pair(request, oracle_mod):
    s = E.scene(*request.param)
    return s, oracle_of(oracle_mod, s)


def test_table(pair, oracle_mod):
    """Distinct buckets, no chain, ptr = 0, 1, 2, ... in ascending entry order, hash_index the oracle's."""
    s, _ = pair
    live = np.flatnonzero(s.hash["ptr"] != -2)
    assert (live < E.TABLES["n_buckets"]).all() and not s.hash["offset"].any()
    pos = s.blocks_of(live)
    assert [oracle_mod.hash_index(*p, E.TABLES["n_buckets"]) for p in pos[:200]] == live[:200].tolist()
    assert np.array_equal(E.hash_index(*pos.T, E.TABLES["n_buckets"]), live)
    ptr = s.hash["ptr"][live]
    assert np.array_equal(ptr[ptr >= 0], np.arange(s.n_alloc)) and s.n_alloc <= E.TABLES["n_blocks"]
    assert set(ptr[ptr < 0]) == {-1}                         # (the ptr -2 ones look like every empty entry)


@pytest.mark.parametrize("pose_name", sorted(E.POSES))
def test_input_condition_and_model(pair, pose_name):
    """Every listed block keeps its corners off camera z in [0, 1e-3) and its /8 coordinates under 2^30 (float64);
    the float64 model that chose the blocks agrees with the oracle's float32 projection on every one of them, and no
    box starts below the LDS rows (uly <= H/8)."""
    s, o = pair
    _, _, nrows = E.region(s.W, s.H)
    for fam in E.FAMILIES:
        ids = s.fam[(pose_name, fam)]
        g = s.project(ids, pose_name)
        assert g["admissible"].all(), fam
        b = boxes(o, s, ids, pose_name)
        has_block = s.hash["ptr"][ids] >= 0
        assert np.array_equal(b["valid"], g["valid"] & has_block), fam
        assert np.array_equal(b["box"][b["valid"]], g["box"][b["valid"]]), fam
        assert (b["box"][b["valid"], 1] <= s.H // E.SUB).all() and s.H // E.SUB < max(nrows, 1)


@pytest.mark.parametrize("pose_name", sorted(E.POSES))
def test_far(pair, pose_name):
    s, o = pair
    ids = s.fam[(pose_name, "far")]
    b = boxes(o, s, ids, pose_name)
    rc, rr, nrows = E.region(s.W, s.H)
    v, box = b["valid"], b["box"]
    inner = v & (box[:, 0] > 0) & (box[:, 1] > 0) & (box[:, 2] < s.W // E.SUB) & (box[:, 3] < s.H // E.SUB)
    assert inner.any() or min(s.W, s.H) // E.SUB < 3        # one or two pixels of the projection, + floor / ceil
    assert (b["w"][inner] <= 3).all() and (b["h"][inner] <= 3).all()
    assert (b["z"][v, 0] > 1.5).all()
    assert (~v).sum() == 2                                   # wholly outside the left and the top border: ulx > lrx
    assert (v & (box[:, 0] == 0)).any() and (v & (box[:, 1] == 0)).any()           # half outside them
    assert b["clamp_w"].sum() == 2 and b["clamp_h"].sum() == 2                    # half and wholly outside right / bottom
    assert (box[b["clamp_w"], 0] == s.W // E.SUB).any() and (box[b["clamp_h"], 1] == s.H // E.SUB).any()
    img, total = expected(o, s, ids, E.POSES[pose_name])
    assert (img[:rr, :rc, 1] > E.VERY_CLOSE).all()           # the blocks tile the /8 region
    assert total == b["need"].sum()


@pytest.mark.parametrize("pose_name", sorted(E.POSES))
def test_near(pair, pose_name):
    s, o = pair
    ids = s.fam[(pose_name, "near")]
    b = boxes(o, s, ids, pose_name)
    rc, rr, nrows = E.region(s.W, s.H)
    assert b["valid"].all() and (b["z"][:, 0] < 0.3).all()
    assert b["past_rc"].sum() >= 10 and b["under_rr"].sum() >= 10 and b["clamp_w"].sum() >= 5 and b["clamp_h"].sum() >= 5
    img, _ = expected(o, s, ids, E.POSES[pose_name])
    written = img[..., 1] > E.VERY_CLOSE
    assert written[:, rc:].any() and written[rr:nrows].any()
    if (s.W, s.H) in E.BIG_SIZES or s.W == 200:
        assert b["below_thread"].sum() >= 10 and b["below_queued"].sum() >= 10
        assert written[nrows:].any() and written[nrows:, rc:].any()
    else:
        assert nrows == s.H and not b["below"].any()         # ed_nrows' cap: no rows below


@pytest.mark.parametrize("pose_name", sorted(E.POSES))
def test_straddle(pair, pose_name):
    s, o = pair
    ids = s.fam[(pose_name, "straddle")]
    b = boxes(o, s, ids, pose_name)
    g = s.project(ids, pose_name)
    ptr = s.hash["ptr"][ids]
    assert (ptr == -1).sum() >= 1 and (ptr == -2).sum() >= 1 and not b["valid"][ptr < 0].any()
    assert g["valid"][ptr < 0].all()                         # (they would have a box)
    listed = np.concatenate([ids, [int(np.flatnonzero(s.hash["ptr"] == -2)[0])]]).astype(np.int32)     # + an empty entry: ptr -2
    img, _ = expected(o, s, listed, E.POSES[pose_name])
    assert_bit_exact("ptr < 0 entries add nothing", img, expected(o, s, ids[ptr >= 0], E.POSES[pose_name])[0])
    have = ptr >= 0
    assert (have & (g["nbehind"] == 8)).any() and not b["valid"][g["nbehind"] == 8].any()
    raised = have & b["valid"] & (g["zfront"][:, 0] < E.VERY_CLOSE) & (g["zfront"][:, 1] >= E.VERY_CLOSE)
    assert raised.any() and (b["z"][raised, 0] == E.VERY_CLOSE).all() and (b["z"][raised, 1] > E.VERY_CLOSE).all()
    if pose_name == "tilted":
        for k in range(1, 8):
            assert (have & (g["nbehind"] == k)).any(), f"no block with {k} corners behind the camera plane"
        assert (have & b["valid"] & (g["nbehind"] > 0) & (g["nbehind"] < 8)).sum() >= 4
        close = have & (g["nbehind"] < 8) & (g["zfront"][:, 1] < E.VERY_CLOSE)
        assert (close & b["valid"]).any()                    # kept: the zmax < VERY_CLOSE rejection cannot fire
        assert (b["z"][close & b["valid"]] == E.VERY_CLOSE).all()
    else:
        assert set(g["nbehind"]) <= {0, 8}                   # corners on multiples of the block size (ed_cases.py)


@pytest.mark.parametrize("pose_name", sorted(E.POSES))
@pytest.mark.parametrize("size", [p for p in SCENES if p[:2] not in E.SMALL_SIZES], ids=lambda p: f"{p[0]}x{p[1]}")
def test_wide_row(oracle_mod, size, pose_name):
    s = E.scene(*size)
    o = oracle_of(oracle_mod, s)
    ids = s.fam[(pose_name, "wide")]
    b = boxes(o, s, ids, pose_name)
    rc, rr, nrows = E.region(s.W, s.H)
    row = s.wide_row[pose_name]
    assert 0 <= row < rr
    covers = b["valid"] & (b["box"][:, 1] <= row) & (b["box"][:, 3] >= row)
    assert (covers & (b["w"] > E.ED_WIDE)).sum() > E.ED_QUEUE + 4        # the queue overflows: segments filled by their thread
    assert (covers & (b["w"] == E.ED_WIDE)).sum() >= 1 and (covers & (b["w"] == E.ED_WIDE + 1)).sum() >= 1
    assert len(ids) <= E.LDS_MAX_N and E.WIDE_BOXES + 8 <= E.LDS_MAX_N   # (on the LDS path under TFUSION_ED_LDS_MAX_N=512 too)


def test_count_lists(pair):
    s, _ = pair
    for pn in E.POSES:
        assert len(np.union1d(s.fam[(pn, "far")], s.fam[(pn, "near")])) < 511 or (s.W, s.H) not in E.BIG_SIZES
        for n, fam in zip(E.COUNTS, E.COUNT_FAMILIES):
            for order in E.ORDERS:
                ids = s.ordered(pn, fam, order)
                assert len(ids) == n and set(ids) <= set(s.fam[(pn, "far")]) | set(s.fam[(pn, "near")])
        a, r, sh = (s.ordered(pn, "near", k) for k in E.ORDERS)
        assert np.array_equal(a, np.sort(a)) and np.array_equal(r, a[::-1]) and np.array_equal(np.sort(sh), a)
        assert not np.array_equal(sh, a) and not np.array_equal(sh, r)
    assert E.LDS_MAX_N - 1 in E.COUNTS and E.LDS_MAX_N in E.COUNTS and E.LDS_MAX_N + 1 in E.COUNTS


@pytest.mark.parametrize("order", E.ORDERS)
@pytest.mark.parametrize("pose_name", sorted(E.POSES))
def test_caps(oracle_mod, pose_name, order):
    """Each cap of cap_points drops exactly the entries it is named for: the oracle's image is the fill of the kept
    boxes and nothing else, at 64x48 and 36x28."""
    for W, H in E.BIG_SIZES:
        s = E.scene(W, H)
        ids = s.ordered(pose_name, "cap", order)
        b = boxes(oracle_of(oracle_mod, s), s, ids, pose_name)
        need = b["need"]
        caps = E.cap_points(need, b["box"], b["z"], W, H)
        off = np.cumsum(need) - need
        total = int(need.sum())
        assert all(caps[k] is not None for k in E.CAP_NAMES)
        for name in E.CAP_NAMES:
            cap = caps[name]
            first, kept = E.cap_expect(name, need, cap)
            img, n_total = expected(oracle_of(oracle_mod, s, max_render_blocks=cap), s, ids, E.POSES[pose_name])
            assert_bit_exact(f"{W}x{H} {name}: the oracle's image is the kept boxes'", img, E.fill(b["box"], b["z"], kept, W, H))
            assert n_total == min(total, cap)
            if name == "total_eq_cap":
                assert first is None and cap == total
            elif name in ("total_eq_cap_plus_1", "first_drop_last"):
                assert total == cap + 1 and first == len(ids) - 1
            elif name in ("first_drop_255", "first_drop_256"):
                assert first == int(name[-3:]) and not kept[first:].any()
            elif name == "exact_fit":
                assert off[first - 1] + need[first - 1] == cap and kept[first - 1] and 0 < first < len(ids) - 1
                kept[first - 1] = False                      # the entry that fits exactly decides pixels on its own
                assert not np.array_equal(img, E.fill(b["box"], b["z"], kept, W, H))
            else:
                assert need[first] >= 2 and need[first + 1] == 1 and off[first] + 1 <= cap and not kept[first + 1]
        assert len({caps[k] for k in E.CAP_NAMES}) >= 6


@pytest.mark.parametrize("view", VIEWS, ids=lambda v: f"{v[0]}x{v[1]}")
def test_view_lists(oracle_mod, view):
    """What a free view's scan lists of each family (checkBlockVisibility: a corner inside the image): enough of the
    near boxes to reach past the /8 columns and under the /8 rows, straddling blocks, wide segments in one row.
    More than ED_QUEUE wide segments in a row cannot be seen at once at these sizes; the stage and engine entry points
    run that case."""
    s = E.scene(*view)
    o = oracle_of(oracle_mod, s)
    rc, rr, nrows = E.region(s.W, s.H)
    for pn, pose in E.POSES.items():
        for fam in ("near", "straddle", "wide"):
            ids = s.fam[(pn, fam)]
            lst = V.visible_list(o, s.hash_only(ids), pose)
            assert set(lst) <= set(ids[s.hash["ptr"][ids] >= 0])
            b = boxes(o, s, lst, pn)
            if fam == "near":
                assert len(lst) >= 15 and b["past_rc"].sum() >= 3 and b["under_rr"].sum() >= 3
            elif fam == "straddle":
                assert len(lst) >= 2 and (pn == "identity" or (s.project(lst, pn)["nbehind"] > 0).any())
            else:
                assert (b["valid"] & (b["w"] > E.ED_WIDE)).sum() >= 5


def test_frame_injection(oracle_mod):
    """The fused frame path's case: frames 2 and 3 track with the injected blocks, the blocks stay listed after frame
    2, frame 2's range image differs from the plain run's outside the /8 region, the threshold between the visible
    counts before and after makes frame 2 the first on the atomic path, and the capped variant's cap is met exactly by
    an entry whose box alone decides pixels the rays read: without it the raycast differs."""
    O = oracle_mod
    W, H = E.FRAME_SIZE
    rc, rr, nrows = E.region(W, H)
    seq = E.frame_sequence()
    o, state, entries = E.frame_setup(O)
    n1 = o.counters()["noVisibleEntries"]
    assert len(entries) >= 30 and state["counters"][2] == n1 + len(entries)
    assert state["counters"][0] == o.counters()["lastFreeBlockId"] - len(entries)
    plain = O.Oracle(O.default_params(**E.frame_params()))
    plain.copy_state_from(o)
    E.frame_load(o, state)
    assert o(seq[2]) and plain(seq[2])
    assert np.isin(entries, o.visible_ids()).all()
    d = (o.range_image() != plain.range_image()).any(axis=2)
    assert d[rr:].sum() + d[:rr, rc:].sum() >= 50
    n2 = o.counters()["noVisibleEntries"]
    assert n1 <= E.frame_threshold(n1, len(entries)) < n2
    assert o(seq[3])
    # the capped variant
    cap, k = E.frame_cap()
    oc, state, entries = E.frame_setup(O, max_render_blocks=cap, **E.STILL)
    E.frame_load(oc, state)
    assert oc(seq[2])
    vis, need, box, z = E.frame_tiles(O, oc)
    off = np.cumsum(need) - need
    assert vis[k] in entries and off[k] + need[k] == cap and oc.counters()["noTotalBlocks"] == cap
    kept, _ = E.serial_cap(need, cap)
    img = oc.range_image()
    assert_bit_exact("capped frame 2", img, E.fill(box, z, kept, W, H))
    kept[k] = False
    pose = oc.pose()
    oc.raycast(pose, 1)
    with_k = oc.raycast_result()
    oc.upload_range_image(E.fill(box, z, kept, W, H))
    oc.raycast(pose, 1)
    assert (oc.raycast_result().view(np.uint32) != with_k.view(np.uint32)).sum() > 100
