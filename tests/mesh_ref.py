"""CPU restatement of mesh extraction (DESIGN.md §Mesh extraction) in numpy, float32 throughout.

Marching tetrahedra on the Kuhn split of every voxel cube of every live hash entry.  Everything here
is derived from the rule, independently of the kernel (topfusion_amd/csrc/tf_mesh.hip): the case
triangles come from the inside set, and their orientation from exact integer geometry -- the
triangle through the edge MIDPOINTS (doubled integer coordinates) must have its right-hand normal
pointing from the inside corners' centroid to the outside corners' -- never from interpolated floats.

    extract(hash, vba, voxel_size, n_buckets) -> (n, 3, 3) float32, in the specified order
"""
import itertools

import numpy as np

from vbh_ref import find_live

PERMS = ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))   # xyz xzy yxz yzx zxy zyx


def tet_corners(k):
    """The four corners of tetrahedron k as integer offsets in the cube, (4, 3)."""
    a, b, _ = PERMS[k]
    c = np.zeros((4, 3), np.int64)
    c[1, a] = 1
    c[2, a] = 1
    c[2, b] = 1
    c[3] = 1
    return c


def case_triangles(k, m):
    """Triangles of tetrahedron k for the inside set m (bit i = corner i inside): a list of triangles,
    each three edges (lo corner, hi corner) of the tetrahedron, oriented towards the outside."""
    inside = [i for i in range(4) if m >> i & 1]
    outside = [i for i in range(4) if not m >> i & 1]
    if len(inside) in (0, 4):
        return []
    if len(inside) == 1:
        i = inside[0]
        tris = [[(i, j) for j in outside]]
    elif len(inside) == 3:
        i = outside[0]
        tris = [[(i, j) for j in inside]]
    else:
        (i, j), (p, q) = inside, outside
        quad = [(i, p), (i, q), (j, q), (j, p)]
        tris = [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    c2 = 2 * tet_corners(k)                                  # doubled: midpoints are integers
    to_out = 2 * (len(inside) * c2[outside].sum(0) - len(outside) * c2[inside].sum(0))   # direction only
    out = []
    for t in tris:
        mid = [(c2[u] + c2[v]) // 2 for u, v in t]
        n = np.cross(mid[1] - mid[0], mid[2] - mid[0])
        s = int(n @ to_out)
        assert s != 0, (k, m, t)
        if s < 0:
            t = [t[0], t[2], t[1]]
        out.append([(min(u, v), max(u, v)) for u, v in t])
    return out


def _tiles(h, vba, n_buckets, live):
    """(n, 9, 9, 9) sdf and w arrays, indexed [z, y, x], of each live entry's cube corners: its own
    block and the seven neighbours, each found as findVoxel does (vbh_ref.find_live; a missing block reads as
    Voxel_s(): sdf 32767, w 0)."""
    v = vba.reshape(-1, 8, 8, 8)
    sdf = np.full((len(live), 16, 16, 16), 32767, np.int32)
    w = np.zeros((len(live), 16, 16, 16), np.int32)
    cache = {}
    for n, e in enumerate(live):
        bx, by, bz = int(h["x"][e]), int(h["y"][e]), int(h["z"][e])
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            if (dx, dy, dz) == (0, 0, 0):
                p = int(h["ptr"][e])
            else:
                key = (bx + dx, by + dy, bz + dz)
                if key not in cache:
                    cache[key] = find_live(h, n_buckets, key)[1]
                p = cache[key]
            if p >= 0:
                sl = (n, slice(8 * dz, 8 * dz + 8), slice(8 * dy, 8 * dy + 8), slice(8 * dx, 8 * dx + 8))
                sdf[sl] = v["sdf"][p]
                w[sl] = v["w"][p]
    return sdf[:, :9, :9, :9], w[:, :9, :9, :9]


def _tables():
    """Per tetrahedron k: corner offsets (4, 3); per (k, case): triangle count and the (lo, hi)
    corners of each triangle vertex, (6, 16, 2, 3, 2)."""
    corners = np.stack([tet_corners(k) for k in range(6)])
    ntri = np.zeros((6, 16), np.int64)
    edges = np.zeros((6, 16, 2, 3, 2), np.int64)
    for k in range(6):
        for m in range(16):
            t = case_triangles(k, m)
            ntri[k, m] = len(t)
            for i, tri in enumerate(t):
                edges[k, m, i] = tri
    return corners, ntri, edges


def extract(h, vba, voxel_size, n_buckets, chunk=64, stats=None):
    """The triangle list of the scene (hash table `h`, voxels `vba`, structured arrays as
    topfusion_amd.topfu.HASH_DTYPE / VOXEL_DTYPE), (n, 3, 3) float32.  stats (dict, optional)
    receives 'cases' (the set of (tetrahedron, case) pairs met) and 't' (the set {0.0, 1.0} & met)."""
    vs = np.float32(voxel_size)
    corners, ntri, edges = _tables()
    live = np.nonzero(h["ptr"] >= 0)[0]
    out = []
    cases, tset = set(), set()
    zz, yy, xx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")   # voxel = x + 8y + 64z
    local = np.stack([xx, yy, zz], -1).reshape(512, 3)
    for c0 in range(0, len(live), chunk):
        ent = live[c0:c0 + chunk]
        sdf, w = _tiles(h, vba, n_buckets, ent)
        n = len(ent)
        valid = np.ones((n, 8, 8, 8), bool)
        for dz, dy, dx in itertools.product((0, 1), repeat=3):
            valid &= w[:, dz:dz + 8, dy:dy + 8, dx:dx + 8] > 0
        valid = valid.reshape(n, 512)
        g0 = np.stack([h["x"][ent], h["y"][ent], h["z"][ent]], -1).astype(np.int64)[:, None, :] * 8 + local[None]
        tri = np.zeros((n, 512, 6, 2, 3, 3), np.float32)
        keep = np.zeros((n, 512, 6, 2), bool)
        for k in range(6):
            s = np.stack([sdf[:, c[2]:c[2] + 8, c[1]:c[1] + 8, c[0]:c[0] + 8].reshape(n, 512) for c in corners[k]], -1)
            m = ((s < 0) << np.arange(4)).sum(-1)                       # (n, 512)
            m = np.where(valid, m, 0)
            cases |= {(k, int(v)) for v in np.unique(m) if ntri[k, v]}
            e = edges[k][m]                                             # (n, 512, 2, 3, 2)
            lo, hi = e[..., 0], e[..., 1]
            sidx = np.broadcast_to(s[:, :, None, None, :], lo.shape + (4,))
            sp = np.take_along_axis(sidx, lo[..., None], -1)[..., 0]
            sq = np.take_along_axis(sidx, hi[..., None], -1)[..., 0]
            on = np.arange(2)[None, None, :] < ntri[k][m][..., None]    # (n, 512, 2)
            den = np.where(on[..., None], sp - sq, 1)
            t = (sp.astype(np.float32) / den.astype(np.float32)).astype(np.float32)
            tset |= {float(v) for v in (0.0, 1.0) if np.any(on[..., None] & (t == np.float32(v)))}
            p = corners[k][lo]                                          # (n, 512, 2, 3, 3)
            d = corners[k][hi] - p
            gp = (g0[:, :, None, None, :] + p).astype(np.float32)
            moved = ((gp + t[..., None]).astype(np.float32) * vs).astype(np.float32)
            fixed = (gp * vs).astype(np.float32)
            tri[:, :, k] = np.where(d == 1, moved, fixed)
            keep[:, :, k] = on
        out.append(tri[keep])
    if stats is not None:
        stats["cases"] = cases
        stats["t"] = tset
    return np.concatenate(out).reshape(-1, 3, 3) if out else np.zeros((0, 3, 3), np.float32)


def weld(tris):
    """Vertices welded by exact bit equality: (vertices (m, 3) float32, faces (n, 3) int)."""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    keys = t.view(np.uint32).reshape(-1, 3)
    uniq, inv = np.unique(keys, axis=0, return_inverse=True)
    return uniq.view(np.float32).reshape(-1, 3), inv.reshape(-1, 3)


# ---- the test scenes ----------------------------------------------------------------------------
def sphere_scene(hash_dtype, voxel_dtype, n_buckets, n_excess, n_blocks, build_hash, r=9.3,
                 centre=(16.37, 15.61, 16.23)):
    """A sphere of radius r voxels inside 4 x 4 x 4 blocks at the origin: sdf = clamp(round((d - r) / 4
    * 32767)), w = 1 where |d - r| <= 3 voxels, Voxel_s() elsewhere.  Returns (hash, vba)."""
    pos = np.array(list(itertools.product(range(4), repeat=3)), np.int64)
    h, _, _ = build_hash(pos, n_buckets, n_excess, hash_dtype)
    vba = np.zeros(n_blocks * 512, voxel_dtype)
    vba["sdf"] = 32767
    v = vba.reshape(-1, 8, 8, 8)
    zz, yy, xx = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    for i, b in enumerate(pos):
        d = np.sqrt((b[0] * 8 + xx - centre[0]) ** 2 + (b[1] * 8 + yy - centre[1]) ** 2 + (b[2] * 8 + zz - centre[2]) ** 2)
        s = np.clip(np.rint((d - r) / 4 * 32767), -32767, 32767).astype(np.int16)
        near = np.abs(d - r) <= 3
        v["sdf"][i] = np.where(near, s, 32767)
        v["w"][i] = near
    return h, vba


def random_scene(hash_dtype, voxel_dtype, n_buckets, n_excess, n_blocks, build_hash, positions, seed=11, fill=0.6):
    """`fill` of the block positions allocated, VBA ptrs shuffled, sdf random over the short range with
    0 and +-32767 over-represented, w from {0, 0, 1, 5}.  Returns (hash, vba)."""
    rng = np.random.default_rng(seed)
    positions = np.asarray(positions, np.int64)
    pos = positions[rng.random(len(positions)) < fill]
    h, entry, _ = build_hash(pos, n_buckets, n_excess, hash_dtype)
    perm = rng.permutation(n_blocks)[:len(pos)]                    # block i's voxels live in VBA block perm[i]
    h["ptr"][entry] = perm
    vba = np.zeros(n_blocks * 512, voxel_dtype)
    sdf = rng.integers(-32768, 32768, vba.size).astype(np.int16)
    pick = rng.random(vba.size)
    sdf[pick < 0.08] = 0
    sdf[(pick >= 0.08) & (pick < 0.14)] = 32767
    sdf[(pick >= 0.14) & (pick < 0.20)] = -32767
    vba["sdf"] = sdf
    vba["w"] = rng.choice(np.array([0, 0, 1, 5], np.uint8), vba.size)
    return h, vba


# ---- the scenes both test files use, built and meshed once per session -----------------------------
VOXEL_SIZE = 0.005
SPHERE_R, SPHERE_C = 9.3, (16.37, 15.61, 16.23)
SMALL = dict(n_buckets=4096, n_excess=512, n_blocks=128)            # the sphere's context
RANDOM = dict(n_buckets=16, n_excess=512, n_blocks=128)             # most blocks chained in excess entries
RANDOM_SEED = 22                                                    # a seed whose valid cubes meet all 84 (tetrahedron, case) pairs

_cache = {}


def _case(name):
    if name not in _cache:
        from topfusion_amd import synth
        from topfusion_amd.topfu import HASH_DTYPE, VOXEL_DTYPE
        if name == "sphere":
            cfg = SMALL
            h, vba = sphere_scene(HASH_DTYPE, VOXEL_DTYPE, build_hash=synth.build_hash, r=SPHERE_R, centre=SPHERE_C, **cfg)
        else:
            cfg = RANDOM
            pos = np.array(list(itertools.product(range(-2, 2), repeat=3)))    # straddles the origin: negative blocks too
            h, vba = random_scene(HASH_DTYPE, VOXEL_DTYPE, build_hash=synth.build_hash, positions=pos, seed=RANDOM_SEED, **cfg)
        stats = {}
        tris = extract(h, vba, VOXEL_SIZE, cfg["n_buckets"], stats=stats)
        for a in (h, vba, tris):
            a.setflags(write=False)
        _cache[name] = (h, vba, tris, stats)
    return _cache[name]


def sphere_case():
    """(hash, vba, reference triangles, stats) of the closed sphere (context capacities SMALL)."""
    return _case("sphere")


def random_case():
    """... of the random scene (context capacities RANDOM)."""
    return _case("random")
