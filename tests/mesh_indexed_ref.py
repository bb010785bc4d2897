"""CPU restatement of the indexed mesh extraction (DESIGN.md §Mesh extraction, indexed) in numpy, written
from the specification and not from the kernels.

Triangles, their order, their values and the case tables are mesh_ref's / mesh_attr_ref's.  This module
derives on its own, per triangle vertex, the Kuhn edge (p, d) it lies on, the hash entry that owns the
edge (the live entry of block floor(p / 8), by findVoxel's walk: vbh_ref.find_live), the vertex order (owner entry,
p's voxel index in the owner block, direction code) and from that the vertex table and the index buffer.

    indexed(hash, vba, voxel_size, n_buckets, rgb=None) -> (vertices (nv, 3) f32, indices (nt, 3) u32,
                                                          normals (nv, 3) f32, colours (nv, 4) u8 | None)
"""
import itertools

import numpy as np

import mesh_attr_ref as A
import mesh_ref as M
from vbh_ref import find_live


def triangle_edges(h, vba, n_buckets, chunk=64):
    """Per triangle vertex of the extraction, in extraction order (entry, voxel, tetrahedron, triangle of
    the case, vertex): the emitting entry (nt,), the edge's lower end p as a global voxel coordinate
    (nt, 3, 3) and its direction d in {0,1}^3 (nt, 3, 3)."""
    corners, ntri, edges = M._tables()
    live = np.nonzero(h["ptr"] >= 0)[0]
    zz, yy, xx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    local = np.stack([xx, yy, zz], -1).reshape(512, 3)                      # voxel = x + 8y + 64z
    out_e, out_p, out_d = [], [], []
    for c0 in range(0, len(live), chunk):
        ent = live[c0:c0 + chunk]
        n = len(ent)
        sdf, w = M._tiles(h, vba, n_buckets, ent)
        valid = np.ones((n, 8, 8, 8), bool)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            valid &= w[:, dz:dz + 8, dy:dy + 8, dx:dx + 8] > 0
        valid = valid.reshape(n, 512)
        g0 = np.stack([h["x"][ent], h["y"][ent], h["z"][ent]], -1).astype(np.int64)[:, None, :] * 8 + local[None]
        P = np.zeros((n, 512, 6, 2, 3, 3), np.int64)
        D = np.zeros((n, 512, 6, 2, 3, 3), np.int64)
        keep = np.zeros((n, 512, 6, 2), bool)
        for k in range(6):
            s = np.stack([sdf[:, c[2]:c[2] + 8, c[1]:c[1] + 8, c[0]:c[0] + 8].reshape(n, 512) for c in corners[k]], -1)
            m = np.where(valid, ((s < 0) << np.arange(4)).sum(-1), 0)
            e = edges[k][m]                                                 # (n, 512, 2, 3, 2)
            p = corners[k][e[..., 0]]                                       # (n, 512, 2, 3, 3)
            P[:, :, k] = g0[:, :, None, None, :] + p
            D[:, :, k] = corners[k][e[..., 1]] - p
            keep[:, :, k] = np.arange(2)[None, None, :] < ntri[k][m][..., None]
        out_p.append(P[keep])
        out_d.append(D[keep])
        out_e.append(np.broadcast_to(ent[:, None, None, None], keep.shape)[keep])
    if not out_p:
        return np.zeros(0, np.int64), np.zeros((0, 3, 3), np.int64), np.zeros((0, 3, 3), np.int64)
    return np.concatenate(out_e), np.concatenate(out_p), np.concatenate(out_d)


def indexed(h, vba, voxel_size, n_buckets, rgb=None, soup=None, stats=None):
    """The indexed mesh of the scene.  soup: (triangles, normals, colours) of mesh_attr_ref.extract_attr for
    the same scene when the caller has them already.  stats (dict, optional) receives 'owner_dirs' (the set
    of owner block - emitting block offsets met), 'excess_owners' (vertices whose owner entry lies in the
    excess list), 'nv', 'nt'."""
    tris, nrm, col = soup if soup is not None else A.extract_attr(h, vba, rgb, voxel_size, n_buckets)
    ent, P, D = triangle_edges(h, vba, n_buckets)
    nt = len(ent)
    assert nt == len(tris), (nt, len(tris))
    assert ((D == 0) | (D == 1)).all() and (D.sum(-1) > 0).all()
    blk = P // 8                                                            # floor: negative coordinates too
    ub, binv = np.unique(blk.reshape(-1, 3), axis=0, return_inverse=True)
    owner_of = np.array([find_live(h, n_buckets, b)[0] for b in ub], np.int64)
    assert (owner_of >= 0).all(), "an edge whose owner block is not live"
    owner = owner_of[binv.reshape(-1)].reshape(nt, 3) if nt else np.zeros((0, 3), np.int64)
    lp = (P % 8) @ np.array([1, 8, 64])
    dc = D @ np.array([1, 2, 4])
    key = (owner * 512 + lp) * 8 + dc                                       # ascending: owner entry, voxel, direction code
    _, first, inv = np.unique(key.reshape(-1), return_index=True, return_inverse=True)
    indices = inv.reshape(-1, 3).astype(np.uint32)
    pick = lambda a, width, dt: np.ascontiguousarray(a).reshape(-1, width)[first] if nt else np.zeros((0, width), dt)
    vertices = pick(tris, 3, np.float32)
    normals = pick(nrm, 3, np.float32)
    colours = pick(col, 4, np.uint8) if col is not None else None
    # the values are functions of the edge alone: every occurrence carries the same bits
    assert vertices[indices].tobytes() == np.ascontiguousarray(tris).tobytes(), "one edge, two positions"
    assert normals[indices].tobytes() == np.ascontiguousarray(nrm).tobytes(), "one edge, two normals"
    if colours is not None:
        assert colours[indices].tobytes() == np.ascontiguousarray(col).tobytes(), "one edge, two colours"
    if stats is not None:
        eb = np.stack([h["x"][ent], h["y"][ent], h["z"][ent]], -1).astype(np.int64)
        stats["owner_dirs"] = {tuple(int(v) for v in o) for o in np.unique((blk - eb[:, None, :]).reshape(-1, 3), axis=0)}
        stats["excess_owners"] = int((owner_of[np.unique(binv)] >= n_buckets).sum())
        stats["nv"], stats["nt"] = len(vertices), nt
    return vertices, indices, normals, colours


# ---- the dense random scene --------------------------------------------------------------------------
DENSE_SEED = 4                # chosen on the CPU: the coverage asserted in dense_case() holds


def dense_scene(seed=DENSE_SEED):
    """All 4 x 4 x 4 blocks around the origin (negative coordinates too) in M.RANDOM's capacities -- 16
    buckets, so most blocks are chained in excess entries -- VBA pointers shuffled, sdf over the whole short
    range with 0 and +-32767 frequent, w from {0, 1, 1, 5}.  Returns (hash, vba)."""
    from topfusion_amd import synth
    from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
    cfg = M.RANDOM
    rng = np.random.default_rng(seed)
    pos = np.array(list(itertools.product(range(-2, 2), repeat=3)), np.int64)
    h, entry, _ = synth.build_hash(pos, cfg["n_buckets"], cfg["n_excess"], HASH_DTYPE)
    h["ptr"][entry] = rng.permutation(cfg["n_blocks"])[:len(pos)]
    vba = np.zeros(cfg["n_blocks"] * 512, VOXEL_DTYPE)
    sdf = rng.integers(-32768, 32768, vba.size).astype(np.int16)
    pick = rng.random(vba.size)
    sdf[pick < 0.10] = 0
    sdf[(pick >= 0.10) & (pick < 0.16)] = 32767
    sdf[(pick >= 0.16) & (pick < 0.22)] = -32767
    vba["sdf"] = sdf
    vba["w"] = rng.choice(np.array([0, 1, 1, 5], np.uint8), vba.size)
    return h, vba


_cache = {}


def _case(name):
    if name not in _cache:
        stats = {}
        if name == "sphere":
            cfg = M.SMALL
            h, vba, rgb, tris, nrm, col, _ = A.sphere_case()
        else:
            cfg = M.RANDOM
            h, vba = dense_scene()
            rgb = A.colour_plane(vba.size)
            tris, nrm, col = A.extract_attr(h, vba, rgb, M.VOXEL_SIZE, cfg["n_buckets"])
            assert tris.tobytes() == M.extract(h, vba, M.VOXEL_SIZE, cfg["n_buckets"]).tobytes()
        v, i, n, c = indexed(h, vba, M.VOXEL_SIZE, cfg["n_buckets"], rgb, soup=(tris, nrm, col), stats=stats)
        if name == "dense":
            # the coverage this scene exists for
            assert stats["nt"] >= 5000, stats["nt"]
            # the seven owner offsets there are: the block itself and six neighbours ((1, 1, 1) owns nothing of
            # this entry's: its only lattice point in the tile is the cubes' top corner, never an edge's lower end)
            assert stats["owner_dirs"] == set(itertools.product((0, 1), repeat=3)) - {(1, 1, 1)}, stats["owner_dirs"]
            assert stats["excess_owners"] > 0
            assert stats["nv"] > len(M.weld(tris)[0]), "no two distinct edges with bit-equal positions"
        for a in (h, vba, rgb, tris, nrm, col, v, i, n, c):
            a.setflags(write=False)
        _cache[name] = dict(cfg=cfg, hash=h, vba=vba, rgb=rgb, tris=tris, tri_normals=nrm, tri_colours=col, vertices=v, indices=i,
                            normals=n, colours=c, stats=stats)
    return _cache[name]


def sphere_case():
    """mesh_ref's sphere, indexed: a dict of the scene (cfg, hash, vba, rgb), the soup (tris, tri_normals,
    tri_colours) and the indexed mesh (vertices, indices, normals, colours, stats)."""
    return _case("sphere")


def dense_case():
    return _case("dense")
