"""The inputs of tests/test_gpu_alloc_edges.py do what they are for, asserted without a GPU: the plain restatement of
AllocateSceneFromDepth in tests/alloc_cases.py equals the oracle on every case it covers (request types and block
coordinates, then hash, visible types, counters, failure counts and visible list after every call), and each family
reaches, by the restatement's own account, the index edge of topfusion_amd/csrc/tf_scene.hip it is built for -- so an
edit to the cases cannot hollow the GPU tests out.  These are conditions, not measurements."""
import numpy as np
import pytest

import alloc_cases as A
from parity_util import assert_bit_exact, assert_struct_exact

HASH_FIELDS = ["x", "y", "z", "pad", "offset", "ptr"]


def oracle_of(O, c):
    """An oracle of the case's parameters with the case's state, through load_scene_state."""
    o = O.Oracle(O.default_params(**c.kw))
    load_oracle(o, c.state)
    return o


def load_oracle(o, s):
    swap = {}
    if o.params.use_swapping:
        flags = (s["hash"]["ptr"] == -1).astype(np.uint8)          # a swapped-out entry has stored data
        swap = dict(swap_state=s["swap_state"], swap_stored_flags=flags, swap_stored=o.swap_stored())
    o.load_scene_state(s["hash"], o.vba(), s["alloc_list"], s["excess_list"], s["visible_ids"], s["vis_type"], s["counters"],
                       **swap)


def by_name(family, name):
    return next(c for c in A.FAMILIES[family]() if c.name == name)


def ref_cases():
    return [c for c in A.all_cases() if c.ref]


@pytest.mark.parametrize("c", ref_cases(), ids=lambda c: c.name)
def test_restatement_equals_oracle(oracle_mod, c):
    o = oracle_of(oracle_mod, c)
    # the request arrays of the first call, on a second oracle (the accessor's call rebuilds the visible list)
    pose, dists = c.calls[0][:2]
    o2 = oracle_of(oracle_mod, c)
    at, _, bc = o2.alloc_requests(pose, dists)
    r = A.load(A.Ref(c.kw), c.state)
    _, want_at, want_bc, _ = r.requests(pose, dists)
    assert_bit_exact(f"{c.name}: entriesAllocType", want_at, at)
    req = want_at > 0
    assert_bit_exact(f"{c.name}: blockCoords", want_bc[req], bc[req, :3])
    assert (bc[req, 3] == 1).all()
    for k, (pose, dists, only, reset) in enumerate(c.calls):
        tag = f"{c.name} call {k}"
        before = o.counters()
        info = r.alloc(pose, dists, only, reset)
        o.alloc(pose, dists, only_update_visible=only, reset_visible=reset)
        assert_struct_exact(f"{tag} hash", r.hash, o.hash(), HASH_FIELDS)
        assert_bit_exact(f"{tag} visible types", r.vis_type, o.visible_type())
        co = o.counters()
        assert (co["lastFreeBlockId"], co["lastFreeExcessListId"], co["noVisibleEntries"]) == r.counters(), tag
        assert o.alloc_failures() == info["fail"], (tag, o.alloc_failures(), info["fail"])
        assert_bit_exact(f"{tag} visible list", r.visible_ids[:r.n_vis], o.visible_ids())
        assert_bit_exact(f"{tag} free blocks", r.alloc_list, o.alloc_list())
        assert_bit_exact(f"{tag} free excess entries", r.excess_list, o.excess_list())
        if c.kw["use_swapping"]:
            assert_bit_exact(f"{tag} swap states", r.swap_state, o.swap_state())
            assert o.swap_counts()[2] == info["realloc"][0], tag
        if only:                                               # the requests are dropped: nothing handed out
            assert all(co[f] == before[f] for f in ("lastFreeBlockId", "lastFreeExcessListId")) and info["fail"] == (0, 0)
            assert info["n1"] + info["n2"] > 0


def test_identity_rotation_inverse(oracle_mod):
    """Matrix4::inv of [I | t] is [I | -t] exactly for every pose the restatement is used with."""
    for c in ref_cases():
        for pose, *_ in c.calls:
            m = np.zeros((4, 4), np.float32)
            m[:3] = pose; m[3, 3] = 1
            ok, inv = oracle_mod.matrix4_inv(m.T.reshape(16))      # column-major
            want = np.eye(4, dtype=np.float32)
            want[:3, 3] = -pose[:, 3]
            assert ok and np.array_equal(inv.reshape(4, 4).T, want), c.name


# ---- slots -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", (255, 256, 257, 600))
def test_slots_counts(target):
    """Tile 0 alone requests exactly 255, 256, 257 and at least 600 distinct entries; the same image again finds them
    all (257 and more go through the tile's `seen` table); the full image's last run requests nothing and finds at
    least 257 entries in every whole tile."""
    c = by_name("slots", f"slots_{target}")
    infos = c.infos()
    got = A.tile_distinct(c.kw, infos[0]["walk"])
    assert (got[0] == target if target < 600 else got[0] >= 600) and not got[1:].any(), got
    assert A.tile_distinct(c.kw, infos[1]["walk"], "finds")[0] >= target - 3      # (the few chain collisions aside)
    assert infos[-1]["n1"] + infos[-1]["n2"] == 0 and len(c.calls) >= 4
    finds = A.tile_distinct(c.kw, infos[-1]["walk"], "finds")
    assert (finds[[0, 1]] >= A.AR_SLOTS + 1).all(), finds


def test_slots_whole_tile_64x48():
    c = by_name("slots", "slots_600_64x48")
    got = A.tile_distinct(c.kw, c.infos()[0]["walk"])
    assert got[5] >= 600 and got.sum() == got[5]
    assert c.infos()[-1]["n1"] + c.infos()[-1]["n2"] == 0
    assert A.tile_distinct(c.kw, c.infos()[-1]["walk"], "finds")[5] >= 600


def test_slots_shared():
    """One tile overflows its table, its neighbour does not, and they request at least 32 of the same entries; at
    least 16 entries' winners come from another tile than their first requester's."""
    c = by_name("slots", "slots_shared")
    w = c.infos()[0]["walk"]
    got = A.tile_distinct(c.kw, w)
    assert got[0] >= 600 and 0 < got[1] <= 255 and not got[2:].any(), got
    assert len(np.intersect1d(A.tile_entries(c.kw, w, 0), A.tile_entries(c.kw, w, 1))) >= 32
    req = w[w["rtype"] > 0]
    tiles = A.tile_of(c.kw, req["pixel"])
    first, last = {}, {}
    for e, t in zip(req["entry"].tolist(), tiles.tolist()):
        first.setdefault(e, t)
        last[e] = t
    assert sum(first[e] != last[e] for e in first) >= 16


def test_slots_type2():
    """Nearly every bucket is taken, so nearly all requests are chain-end requests; the whole tiles request more distinct
    entries than their table holds, most of them of type 2."""
    c = by_name("slots", "slots_type2")
    info = c.infos()[0]
    assert (c.state["hash"]["ptr"][:c.kw["n_buckets"]] >= 0).sum() >= 500       # of 512
    w = info["walk"]
    for tile in (0, 1):
        ents = A.tile_entries(c.kw, w, tile)
        assert len(ents) >= A.AR_SLOTS + 1
        assert (info["alloc_type"][ents] == 2).sum() > (len(ents) - A.AR_SLOTS) + len(ents) // 2


# ---- steps -----------------------------------------------------------------------------------------------------------
def test_steps_mu_bound():
    lo, hi = A.mu_largest()
    assert A.mu_accepted(lo) and not A.mu_accepted(hi) and np.nextafter(np.float32(lo), np.float32(1)) == np.float32(hi)


@pytest.mark.parametrize("n", list(A.STEP_MUS) + ["top"])
def test_steps_max(n):
    """The largest noSteps of the image is the one the case is named for (the top one at least 56, inside the key's
    six bits), and from two steps on at least 16 entries are won by a step whose predecessor was in the same block."""
    c = by_name("steps", f"steps_{n}")
    info = c.infos()[0]
    w = info["walk"]
    top = int(w["step"].max()) + 1
    assert (56 <= top <= 63) if n == "top" else top == n, top
    if top >= 2:
        winners = info["last"][info["last"] >= 0]
        later = winners[w["step"][winners] > 0]
        prev = later - 1
        same = (w["pixel"][prev] == w["pixel"][later]) & (w["x"][prev] == w["x"][later]) & (w["y"][prev] == w["y"][later]) \
            & (w["z"][prev] == w["z"][later])
        assert same.sum() >= 16
    if top > A.BATCH:
        assert (w["step"][info["last"][info["last"] >= 0]] >= A.BATCH).sum() >= 16     # winners from a later batch


def test_steps_own_bucket_collisions():
    """256 buckets, 17 steps: at least 16 pixels have two steps of their own in one bucket with different blocks."""
    c = by_name("steps", "steps_17_256")
    w = c.infos()[0]["walk"]
    n = 0
    for p in np.unique(w["pixel"]):
        s = w[w["pixel"] == p]
        seen = {}
        for e, b in zip(s["entry"].tolist(), zip(s["x"].tolist(), s["y"].tolist(), s["z"].tolist())):
            seen.setdefault(e, set()).add(b)
        n += any(len(v) > 1 for v in seen.values())
    assert n >= 16


# ---- collide ---------------------------------------------------------------------------------------------------------
def test_collide():
    """The same image frame after frame until nothing is requested, within the cap; in one frame at least 16 entries
    are requested by three or more distinct positions; the table ends with a chain of at least 8 entries."""
    c = by_name("collide", "collide")
    infos = c.infos()
    assert 10 <= len(c.calls) <= A.COLLIDE_CAP and infos[-1]["n1"] + infos[-1]["n2"] == 0
    assert all(i["n1"] + i["n2"] > 0 for i in infos[:-1])
    w = infos[1]["walk"]
    req = w[w["rtype"] > 0]
    positions = {}
    for e, b in zip(req["entry"].tolist(), zip(req["x"].tolist(), req["y"].tolist(), req["z"].tolist())):
        positions.setdefault(e, set()).add(b)
    assert sum(len(v) >= 3 for v in positions.values()) >= 16
    h, nb = A.after(c.kw, c.state, c.calls)[0]["hash"], c.kw["n_buckets"]
    longest = 0
    for b in range(nb):
        n, i = 1, b
        while h["offset"][i] >= 1:
            i, n = nb + h["offset"][i] - 1, n + 1
        longest = max(longest, n)
    assert longest >= 8


# ---- grid ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in A.grid() if hasattr(c, "axis")], ids=lambda c: c.name)
def test_grid_classes(c):
    """At least 16 steps of every class -- found in the bucket, deep in a chain, swapped out; requested in the bucket
    and at a chain end -- on both sides of the block grid's boundary, at least 16 batches of 8 steps with steps on
    both sides, and a request at the table's last entry."""
    w = c.infos()[0]["walk"]
    outside = A.grid_side(c, c.axis, c.side)
    assert set(np.unique(w["xyz"[c.axis]][outside]).tolist()) >= ({-129} if c.side == 0 else {128})
    assert set(np.unique(w["xyz"[c.axis]][~outside]).tolist()) >= ({-128} if c.side == 0 else {127})
    for side in (outside, ~outside):
        for found in (A.FOUND_BUCKET, A.FOUND_CHAIN, A.FOUND_BUCKET_OUT):
            assert ((w["found"] == found) & side).sum() >= 16, (found, int(side[0]))
        for rtype in (1, 2):
            assert ((w["rtype"] == rtype) & side).sum() >= 16, rtype
    batch = w["pixel"].astype(np.int64) * 8 + w["step"] // A.BATCH
    both = np.intersect1d(batch[outside], batch[~outside])
    assert len(both) >= 16
    n_total = c.kw["n_buckets"] + c.kw["n_excess"]
    assert ((w["entry"] == n_total - 1) & (w["rtype"] == 2)).any()
    if c.side == 1:       # blocks of their own where an index formed from coordinate 128 would land, never walked
        alias = np.asarray(c.state["alias"])
        assert len(alias) >= 16 and (c.state["hash"]["ptr"][alias] >= 0).all() and not np.isin(alias, w["entry"][w["rtype"] == 0]).any()
        assert (c.infos()[-1]["vis_type"][alias] == 0).all()
    # the chains are at least 8 deep
    h, nb = c.state["hash"], c.kw["n_buckets"]
    e = int(w["entry"][w["found"] == A.FOUND_CHAIN][0])
    b = A.hash_index(h["x"][e], h["y"][e], h["z"][e], nb)
    n, i = 1, b
    while i != e:
        i, n = nb + h["offset"][i] - 1, n + 1
    assert n >= 8


# ---- skip ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("skip", "skip_alt"))
def test_skip_sides(name):
    """Every value lands on the side of its rejection test it was made for: 0, -1, d < mu, d - mu one step below
    viewFrustum_min and d + mu one step above viewFrustum_max are skipped; the exact fits are walked."""
    c = by_name("skip", name)
    kw = c.kw
    vals = A.skip_values(kw)
    mu, vmin, vmax = (np.float32(kw[k]) for k in ("mu", "viewFrustum_min", "viewFrustum_max"))
    assert [t for _, t in vals] == [False, False, False, True, False, True, False, True]
    assert vals[3][0] - mu == vmin and vals[4][0] - mu < vmin and vals[4][0] == np.nextafter(vals[3][0], np.float32(0))
    assert vals[5][0] + mu == vmax and vals[6][0] + mu > vmax and vals[6][0] == np.nextafter(vals[5][0], np.float32(9))
    assert 0 < vals[2][0] < mu
    taken = A.segments(kw, A.rt(), c.calls[0][1])[0]
    assert np.array_equal(taken, c.taken) and c.taken.any() and (~c.taken).any()
    walked = np.zeros(taken.size, bool)
    walked[np.unique(c.infos()[0]["walk"]["pixel"])] = True
    assert np.array_equal(walked.reshape(taken.shape), c.taken)


# ---- apply -----------------------------------------------------------------------------------------------------------
def apply_cases():
    return [c for c in A.apply() if hasattr(c, "pair")]


@pytest.mark.parametrize("c", apply_cases(), ids=lambda c: c.name)
def test_apply_failures(c):
    """Per (v0, e0) pair the failure counts the serial loop's definition gives: with enough of the other resource the
    first v0 + 1 requests (or the first e0 + 1 type-2 requests) succeed and the rest fail."""
    info = c.infos()[0]
    n1, n2, (v_free, e_free) = c.n1, c.n2, c.plenty
    assert (info["n1"], info["n2"]) == (n1, n2) and n1 + n2 > 0 and n2 > 0
    f1, f2 = info["fail"]
    v_after, e_after, _ = info["counters"]
    kinds = [info["alloc_type"][t] for t in sorted(info["ok"])]
    oks = [info["ok"][t] for t in sorted(info["ok"])]
    if c.pair.startswith("v0=") and e_free + 1 >= n2:
        assert f1 + f2 == max(0, n1 + n2 - (c.v0 + 1)), (f1, f2)
        assert v_after == max(-1, c.v0 - n1 - n2)
        assert oks == [k <= c.v0 for k in range(n1 + n2)]         # the first v0 + 1 in index order
    elif c.pair.startswith("e0="):
        assert (f1, f2) == (0, max(0, n2 - (c.e0 + 1)))
        assert e_after == max(-1, c.e0 - n2)
    elif c.pair == "excess_first":
        assert f1 == 0 and f2 == n2 - (c.e0 + 1) > 0
        first_fail = oks.index(False)
        assert any(ok and k == 1 for ok, k in zip(oks[first_fail:], kinds[first_fail:])) or n1 == 0
    elif c.pair == "blocks_first":
        assert f1 + f2 > 0 and v_after == -1 and (e_after >= 0 or e_free + 1 < n2)
        first_fail = next(i for i, (ok, k) in enumerate(zip(oks, kinds)) if not ok and k == 1)
        assert f1 > 0 and not any(oks[first_fail:])               # once the blocks are gone nothing succeeds
    assert c.state["alloc_list"].tolist() != sorted(c.state["alloc_list"].tolist())      # non-identity free lists


def test_apply_covers_every_pair():
    names = {c.name for c in apply_cases()}
    for pair in ("v0=-1", "v0=0", "v0=n-2", "v0=n-1", "v0=n", "e0=-1", "e0=0", "e0=n2-2", "e0=n2-1", "e0=n2", "excess_first",
                 "blocks_first"):
        assert f"apply_0x8000+0x2000_{pair}" in names
    for table in ("256+48", "4096+16"):
        for pair in ("v0=-1", "v0=0", "v0=n", "e0=-1", "e0=0", "excess_first", "blocks_first"):
            assert f"apply_{table}_{pair}" in names
    c = by_name("apply", "apply_256+48_excess_first")
    info = c.infos()[0]
    oks = [info["ok"][t] for t in sorted(info["ok"])]
    kinds = [info["alloc_type"][t] for t in sorted(info["ok"])]
    first_fail = oks.index(False)
    assert sum(ok and k == 1 for ok, k in zip(oks[first_fail:], kinds[first_fail:])) >= 16   # type 1 goes on succeeding


def test_apply_chunks():
    """Requests per chunk of 4096 entries: more than 512 in one and none in another (0x8000 + 0x2000), a ragged only
    chunk (256 + 48) and a ragged last chunk (4096 + 16) that hold requests, a type-2 request at the last entry."""
    big = A.chunk_counts(by_name("apply", "apply_0x8000+0x2000_v0=n"))
    assert len(big) == 10 and big.max() > 512 and big.min() == 0, big
    small = A.chunk_counts(by_name("apply", "apply_256+48_v0=n"))
    assert len(small) == 1 and small[0] >= 16 and (256 + 48) % A.CHUNK
    mid = A.chunk_counts(by_name("apply", "apply_4096+16_v0=n"), 1)
    assert len(mid) == 2 and mid[1] >= 1, mid
    last = by_name("apply", "apply_last_entry")
    assert any(i["alloc_type"][-1] == 2 for i in last.infos())


# ---- vis -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [c for c in A.vis() if hasattr(c, "cap") and c.env["TFUSION_VIS_FUSED"] == "1"], ids=lambda c: c.name)
def test_vis_caps(c):
    """The first frame lists exactly VIS_NEED entries (one past a chunk) against caps of need - 2 .. need + 1 and 1;
    from the shifted pose some listed blocks leave the frustum (3 -> 0), and with a binding cap entries that were
    left off the list keep their stale type."""
    infos = c.infos()
    assert infos[0]["need"] == A.VIS_NEED == A.CHUNK + 1
    assert infos[0]["counters"][2] == min(c.cap, A.VIS_NEED)
    listed = infos[0]["listed"][:c.cap]
    assert c.cap == 1 or (infos[1]["vis_type"][listed] == 0).sum() >= 16
    if c.cap < A.VIS_NEED:
        unlisted = infos[0]["listed"][c.cap:]
        untouched = np.setdiff1d(unlisted, infos[1]["walk"]["entry"])
        assert len(untouched) >= 1 and (infos[1]["vis_type"][untouched] == 1).all()
    assert infos[1]["need"] > c.cap and infos[1]["counters"][2] == c.cap
    # entries of type 3 that the capped list of call 1 dropped leave the frustum in call 2: tested although unlisted
    assert c.cap == 1 or infos[2]["off_list_dropped"] >= 16


# ---- swapping --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("swapping_grid_z-", "swapping_grid_x+", "swapping_apply_4096+16"))
def test_swapping_reallocations(name):
    """The ordinary requests take their blocks, then the blocks run out halfway through the re-allocations of the
    swapped-out entries that became visible: at least 8 done, at least 8 refused."""
    c = by_name("swapping", name)
    info = c.infos()[0]
    assert info["fail"][0] == 0
    assert info["realloc"][0] >= 8 and info["realloc"][1] >= 8 and info["counters"][0] == -1
    assert (info["vis_type"] == 2).sum() >= 16


def test_reset_leaves_type3_off_the_list():
    """resetVisibleList drops the list, not the types: from the shifted pose entries still of type 3 leave the
    frustum and must become 0 although no list names them."""
    n = [c.infos()[2]["off_list_dropped"] for c in A.all_cases() if c.name.endswith("+reset")]
    assert len(n) == 7 and all(v >= 16 for v in n), n


def test_variants_present():
    """Every family runs once with onlyUpdateVisibleList, once with resetVisibleList and once under a rotated pose."""
    for fam, f in A.FAMILIES.items():
        names = [c.name for c in f()]
        assert any(n.endswith("+only") for n in names) and any(n.endswith("+rotated") for n in names), fam
        assert fam == "swapping" or any(n.endswith("+reset") for n in names), fam
    assert len(set(A.case_ids())) == len(A.case_ids())
