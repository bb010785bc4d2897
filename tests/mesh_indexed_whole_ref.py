"""CPU restatement of the whole map's indexed mesh (DESIGN.md §Mesh extraction, the whole map, indexed).

No new statement of marching tetrahedra: the two existing specifications compose.  mesh_whole_ref.resolve turns
both tiers into one resolved scene in which every entry keeps its index, position and chain link, and
mesh_indexed_ref.indexed of that scene -- whose owner rule, "the first entry of the block on the hash walk with
ptr >= 0", reads there as "the first entry that resolves" -- is the whole indexed mesh:

    indexed_whole(hash, vba, state, flags, store, voxel_size, n_buckets, maxW) ->
        (vertices (nv, 3) f32, indices (nt, 3) u32, normals (nv, 3) f32)
"""
import numpy as np

import mesh_indexed_ref as X
import mesh_ref as M
import mesh_whole_ref as WR


def indexed_whole(h, vba, state, flags, store, voxel_size, n_buckets, maxW=WR.MAXW, stats=None):
    """The whole indexed mesh.  stats (dict, optional): mesh_indexed_ref.indexed's, on the resolved scene."""
    h2, v2 = WR.resolve(h, vba, state, flags, store, maxW)
    v, i, n, _ = X.indexed(h2, v2, voxel_size, n_buckets, stats=stats)
    return v, i, n


def ownership(h, vba, state, flags, store, n_buckets, maxW=WR.MAXW):
    """Per triangle of the whole reading its emitting entry (nt,) and per triangle vertex the hash entry that
    owns its edge (nt, 3), derived here from the edges' lower ends by the walk of the resolved hash."""
    h2, v2 = WR.resolve(h, vba, state, flags, store, maxW)
    ent, P, _ = X.triangle_edges(h2, v2, n_buckets)
    ub, binv = np.unique((P // 8).reshape(-1, 3), axis=0, return_inverse=True)
    owner_of = np.array([X.find_live(h2, n_buckets, b)[0] for b in ub], np.int64)
    return ent, owner_of[binv.reshape(-1)].reshape(-1, 3)


_cache = {}


def two_tier_indexed(seed=WR.SEED):
    """mesh_whole_ref.two_tier_case(seed) with its whole indexed mesh: the case's dict plus vertices, indices,
    vnormals (per vertex; the case's `normals` are the soup's) and stats.  Computed once, read-only."""
    if seed not in _cache:
        c = dict(WR.two_tier_case(seed))
        stats = {}
        v, i, n = indexed_whole(c["hash"], c["vba"], c["state"], c["flags"], c["store"], M.VOXEL_SIZE, M.RANDOM["n_buckets"], stats=stats)
        for a in (v, i, n):
            a.setflags(write=False)
        c.update(vertices=v, indices=i, vnormals=n, stats=stats)
        _cache[seed] = c
    return _cache[seed]
