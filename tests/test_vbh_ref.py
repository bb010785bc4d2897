"""The rules every test reference shares (tests/vbh_ref.py: the layouts, hashIndex, the chain and the walks over it) held
to the C oracle, to literals on a hand-written table and to each other, and the checkpoint file's one layout
(tests/scene_ckpt_ref.py).  No GPU."""
import itertools

import numpy as np

import alloc_cases as A
import scene_ckpt_ref as R
import scene_map_ref as MR
import scene_resize_ref as Z
import vbh_ref as V
from topfusion_amd import synth, topfu

EDGES = (-32768, -32767, -129, -1, 0, 1, 7, 128, 32766, 32767)
SIZES = (16, 64, 256, 4096, 0x100000)


def test_hash_index_is_the_oracles(oracle_mod):
    pos = np.array(list(itertools.product(EDGES, repeat=3)), np.int64)
    pos = np.concatenate([pos, np.random.default_rng(7).integers(-32768, 32768, (2000, 3))])
    for nb in SIZES:
        got = V.hash_index(pos[:, 0], pos[:, 1], pos[:, 2], nb)
        assert got.dtype == np.int64 and got.shape == (len(pos),)
        assert got.tolist() == [oracle_mod.hash_index(*p, nb) for p in pos.tolist()]
        assert np.array_equal(got, synth.hash_index(pos[:, 0], pos[:, 1], pos[:, 2], nb))
        for p, g in zip(pos[::7], got[::7]):                       # numpy scalars and Python ints: a Python int
            assert type(V.hash_index(*p, nb)) is int and V.hash_index(*p, nb) == V.hash_index(*p.tolist(), nb) == g


def test_dtypes_are_the_librarys_and_the_oracles(oracle_mod):
    for name in ("HASH_DTYPE", "VOXEL_DTYPE"):
        mine = getattr(V, name)
        for other in (getattr(topfu, name), getattr(oracle_mod, name)):
            assert mine.itemsize == other.itemsize and mine.names == other.names
            for f in mine.names:
                assert mine.fields[f][:2] == other.fields[f][:2], (name, f)     # (format, byte offset)
    assert V.reset_entry().tolist() == (0, 0, 0, 0, 0, -2) and V.VOXEL_RESET == 0x00007FFF
    h = V.empty_hash(5)
    assert h.dtype == V.HASH_DTYPE and h.tobytes() == V.reset_entry().tobytes() * 5


# ---- a hand-written table: 16 buckets (entries 0..15) + 16 excess entries (16..31) ----------------------------------------
A3, B3, C3 = (-3, -3, -3), (-3, 2, 0), (-3, 3, 3)              # bucket 3: a chain of three
D6, E6, F6, G6 = (-3, -3, 2), (-3, -2, -1), (-3, 2, 3), (-3, 3, 0)   # bucket 6: the middle one swapped out; G6 not held
H9, L9 = (-3, -1, -3), (-3, 0, 0)                              # bucket 9: H9 twice, a dead copy ahead of the live one; L9 not held
K12 = (-3, -1, 2)                                              # bucket 12: the bucket entry free, its stale offset names K12's
FAR, FAR16 = (40000, 1, 2), (-25536, 1, 2)                     # bucket 11: a coordinate outside int16, and what a short makes of it
NOWHERE = (0, 0, 0)                                            # bucket 0: empty


def hand_table():
    h = V.empty_hash(32)
    h[3], h[21], h[16] = (*A3, 0, 6, 4), (*B3, 0, 1, 5), (*C3, 0, 0, 6)
    h[6], h[18], h[19] = (*D6, 0, 3, 7), (*E6, 0, 4, -1), (*F6, 0, 0, 8)
    h[9], h[26] = (*H9, 0, 11, -1), (*H9, 0, 0, 9)
    h[12], h[24] = (*K12, 0, 9, -2), (*K12, 0, 0, 10)
    h[11] = (*FAR16, 0, 0, 11)
    return h


def test_hand_table_buckets():
    got = [V.hash_index(*p, 16) for p in (A3, B3, C3, D6, E6, F6, G6, H9, L9, K12, FAR, FAR16, NOWHERE)]
    assert got == [3, 3, 3, 6, 6, 6, 6, 9, 9, 12, 11, 11, 0]


def test_chain():
    h = hand_table()
    want = {A3: [3, 21, 16], C3: [3, 21, 16], E6: [6, 18, 19], G6: [6, 18, 19], H9: [9, 26], K12: [12, 24], FAR: [11], NOWHERE: [0]}
    for p, w in want.items():
        assert list(V.chain(h, 16, p)) == w, p


def test_find_live():
    h = hand_table()
    want = {A3: (3, 4), B3: (21, 5), C3: (16, 6), D6: (6, 7), E6: (-1, -1), F6: (19, 8), G6: (-1, -1), H9: (26, 9), L9: (-1, -1),
            K12: (24, 10), FAR: (-1, -1), FAR16: (11, 11), NOWHERE: (-1, -1)}
    for p, w in want.items():
        assert V.find_live(h, 16, p) == w, p
    assert V.find_live(h, 16, (1, 40000, 2)) == V.find_live(h, 16, (1, 2, -32769)) == (-1, -1)


def test_find_held():
    h = hand_table()
    want = {A3: ([3], 3), C3: ([16], 3), E6: ([18], 3), G6: ([], 3), H9: ([9, 26], 2), L9: ([], 2), K12: ([24], 2), NOWHERE: ([], 1)}
    for p, w in want.items():
        assert V.find_held(h, 16, p) == w, p
        # the allocation's walk follows no chain from a free bucket entry: K12 is out of its reach
        assert V.find_held(h, 16, p, from_free_bucket=False) == (([], 0) if p in (K12, NOWHERE) else w), p


def test_probe():
    h = hand_table()
    want = {A3: (3, 0, V.FOUND_BUCKET), B3: (21, 0, V.FOUND_CHAIN), C3: (16, 0, V.FOUND_CHAIN), E6: (18, 0, V.FOUND_CHAIN_OUT),
            F6: (19, 0, V.FOUND_CHAIN), G6: (19, 2, V.FOUND_NONE), H9: (9, 0, V.FOUND_BUCKET_OUT), L9: (26, 2, V.FOUND_NONE),
            K12: (12, 1, V.FOUND_NONE), NOWHERE: (0, 1, V.FOUND_NONE)}
    for p, w in want.items():
        assert V.probe(h, 16, p) == w, p
    assert (V.FOUND_NONE, V.FOUND_BUCKET, V.FOUND_CHAIN, V.FOUND_BUCKET_OUT, V.FOUND_CHAIN_OUT) == (0, 1, 2, 3, 4)
    assert A.lookup is V.probe and A.FOUND_CHAIN_OUT == 4


def test_place_lays_out_what_resize_builds(oracle_mod):
    """scene_resize_ref.made_state's records (about 700 seeded positions, a fifth without a block) go one after another
    into a reset 256 + 768 table: each is found where it went, on the chain of the oracle's bucket, and the table is
    the one scene_resize_ref.resize builds."""
    s = Z.made_state(False)
    nb, ne, nblk = (Z.MADE[k] for k in ("n_buckets", "n_excess", "n_blocks"))
    e = R.records_of(s)["entry"]
    e = e[e["ptr"] >= -1]
    assert 650 < len(e) < 800
    h, excess, last, block = V.empty_hash(nb + ne), np.arange(ne, dtype=np.int32), ne - 1, nblk - 1
    placed = []
    for r in e:
        ptr = -1
        if r["ptr"] >= 0:
            ptr, block = block, block - 1
        t, last = V.place(h, nb, (r["x"], r["y"], r["z"]), ptr, excess, last)
        placed.append((t, ptr))
    for r, (t, ptr) in zip(e, placed):
        pos = (r["x"], r["y"], r["z"])
        assert V.find_held(h, nb, pos)[0] == [t] and V.find_live(h, nb, pos) == ((t, ptr) if ptr >= 0 else (-1, -1))
        assert V.probe(h, nb, pos)[:2] == (t, 0)
        assert next(V.chain(h, nb, pos)) == oracle_mod.hash_index(*pos, nb)
    occupied = len(set(V.hash_index(e["x"], e["y"], e["z"], nb).tolist()))
    assert last == ne - 1 - (len(e) - occupied) and occupied == int((h["ptr"][:nb] >= -1).sum())
    out, report = Z.resize(s, nb, ne, nblk, 64)
    assert h.tobytes() == out["hash"].tobytes()
    assert out["counters"]["lastFreeExcessListId"] == last and report["excess_used"] == len(e) - occupied


def test_probe_finds_what_the_oracle_allocated(oracle_mod):
    """One AllocateSceneFromDepth of a 256 + 48 case whose requests are of both types: probe() finds every position
    the oracle's table then holds, at the oracle's entry."""
    from test_alloc_cases import load_oracle               # (here: importing that module builds every case)
    c = next(c for c in A.apply() if c.name == "apply_256+48_v0=n")
    o = oracle_mod.Oracle(oracle_mod.default_params(**c.kw))
    load_oracle(o, c.state)
    before = o.hash()
    pose, dists, only, reset = c.calls[0]
    o.alloc(pose, dists, only_update_visible=only, reset_visible=reset)
    h, nb = o.hash(), c.kw["n_buckets"]
    new = np.flatnonzero((h["ptr"] >= 0) & (before["ptr"] < -1))
    assert (new < nb).any() and (new >= nb).any()                   # allocated in buckets and at chain ends
    for i in np.flatnonzero(h["ptr"] >= 0):
        assert V.probe(h, nb, (h["x"][i], h["y"][i], h["z"][i]))[:2] == (i, 0), i


# ---- the checkpoint file's layout -----------------------------------------------------------------------------------------
MAPS = ["map0", "map1", "map2", "map3", "map4", "map5"]
LISTS = ["visibleIds", "allocList", "excessList"]
TINY_MAP_BYTES = 2 * 16 * (16 * 12 + 8 * 6 + 4 * 3)


def _layout_of(s):
    rec = R.records_of(s)
    counts = (len(rec), int((rec["entry"]["ptr"] >= 0).sum()), int((rec["hasStoredData"] == 1).sum()))
    return counts, R.layout(s["params"], s["counters"], *counts)


def _tiles(sections, total):
    return [o for _, o, _ in sections] + [total] == np.cumsum([0] + [n for _, _, n in sections]).tolist()


def test_layout_version_1():
    for rgb in (0, 1):
        s = R.tiny_state(voxel_rgb=rgb)
        counts, (version, sections, total) = _layout_of(s)
        assert version == 1 and counts == (4, 2, 0)
        assert [name for name, _, _ in sections] == ["header", "records", "active_blocks"] + LISTS + MAPS
        assert _tiles(sections, total)
        assert total == 296 + 24 * 4 + (4096 if rgb else 2048) * 2 + 4 * (2 + 0 + 5) + TINY_MAP_BYTES
        assert total == len(R.pack(s)) == R.file_size(s["params"], s["counters"], 4, 2)


def test_layout_version_2():
    s = MR.tiny_state()
    counts, (version, sections, total) = _layout_of(s)
    assert version == 2 and counts == (7, 3, 4)
    assert [name for name, _, _ in sections] == ["header", "records", "active_blocks", "stored_blocks"] + LISTS + MAPS
    assert _tiles(sections, total)
    assert total == 304 + 24 * 7 + 2048 * (3 + 4) + 4 * (2 + 1 + 5) + TINY_MAP_BYTES
    data = MR.pack(s)
    assert total == len(data) == MR.file_size(s["params"], s["counters"], 7, 3, 4)
    at = {name: data[o:o + n] for name, o, n in sections}
    assert at["allocList"] == s["allocList"][:1].tobytes() and at["excessList"] == s["excessList"][:5].tobytes()
    assert at["visibleIds"] == s["visibleIds"].tobytes() and at["map5"] == s["maps"][5].tobytes()
    assert at["stored_blocks"] == s["store"].reshape(-1, 512)[[3, 9, 11, 13]].tobytes()
