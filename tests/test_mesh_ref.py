"""The mesh specification on the CPU (tests/mesh_ref.py, DESIGN.md §Mesh extraction): the closed sphere's
reference mesh is watertight, consistently oriented and where it should be; the random scene meets
every case the GPU comparison (tests/test_gpu_mesh.py) must cover; the PLY writer and reader round
trip.  The library is loaded for its host-only PLY writer; nothing here needs a GPU."""
import numpy as np

import mesh_ref as M


def _nondegenerate(faces):
    f = faces
    return f[(f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])]


def test_sphere_closed_and_oriented():
    """After welding by bit equality every directed edge of a non-degenerate triangle occurs once and
    has exactly one reversed twin: a closed 2-manifold, consistently oriented."""
    _, _, tris, _ = M.sphere_case()
    assert len(tris) > 2000
    _, faces = M.weld(tris)
    f = _nondegenerate(faces)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    key = e[:, 0] << 32 | e[:, 1]
    rev = e[:, 1] << 32 | e[:, 0]
    uniq, cnt = np.unique(key, return_counts=True)
    assert (cnt == 1).all(), f"{(cnt > 1).sum()} directed edges used more than once"
    assert np.array_equal(uniq, np.unique(rev)), "a directed edge without its reversed twin"


def test_sphere_volume_and_vertices():
    """Signed volume positive (normals point out of the sphere, towards sdf >= 0) and between the
    volumes of spheres of radius r -+ 2 voxels; every vertex on a lattice edge or diagonal (<= sqrt 3
    voxels) whose ends straddle the sphere."""
    _, _, tris, _ = M.sphere_case()
    t = tris.astype(np.float64) / M.VOXEL_SIZE                     # voxel units
    vol = np.einsum("ni,ni->n", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6
    ball = lambda r: 4 / 3 * np.pi * r ** 3
    print(f"signed volume {vol:.2f} voxels^3, ball(r) {ball(M.SPHERE_R):.2f}")
    assert ball(M.SPHERE_R - 2) < vol < ball(M.SPHERE_R + 2)
    p = t.reshape(-1, 3)
    near = np.abs(p - np.rint(p)) < 1e-4                           # coordinates on the lattice
    lo = np.where(near, np.rint(p), np.floor(p))
    hi = np.where(near, np.rint(p), np.ceil(p))
    frac = np.where(near, np.nan, p - lo)
    spread = np.nanmax(frac, 1) - np.nanmin(frac, 1)               # the moving axes share one t
    assert np.all(np.isnan(spread) | (spread < 1e-4))
    assert np.all((hi - lo).max(1) <= 1)
    c = np.array(M.SPHERE_C)
    dlo = np.linalg.norm(lo - c, axis=1) - M.SPHERE_R
    dhi = np.linalg.norm(hi - c, axis=1) - M.SPHERE_R
    assert np.all(np.minimum(dlo, dhi) <= 1e-3) and np.all(np.maximum(dlo, dhi) >= -1e-3)


def test_random_scene_covers_every_case():
    """All 6 x 14 non-empty (tetrahedron, case) pairs and vertices with t == 0 and t == 1 occur in the
    random scene, so the GPU comparison against it covers them; so do blocks in excess entries and
    missing neighbours."""
    h, _, tris, stats = M.random_case()
    want = {(k, m) for k in range(6) for m in range(1, 15)}
    assert stats["cases"] == want, sorted(want - stats["cases"])
    assert stats["t"] == {0.0, 1.0}
    assert len(tris) > 100
    live = np.nonzero(h["ptr"] >= 0)[0]
    assert (live >= M.RANDOM["n_buckets"]).sum() >= 4              # several blocks sit in excess entries
    blocks = {(int(h["x"][e]), int(h["y"][e]), int(h["z"][e])) for e in live}
    dirs = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)][1:]
    for d in dirs:                                                 # each direction both present and missing
        there = [tuple(np.add(b, d)) in blocks for b in blocks]
        assert any(there) and not all(there), d


def test_case_rule_orientation_is_consistent():
    """The rule-derived orientation makes neighbouring tetrahedra agree: on a plane sdf = x + y + z - c
    through one cube every triangle's normal has a positive component along (1, 1, 1)."""
    corners = np.stack([M.tet_corners(k) for k in range(6)])
    for c in (0.5, 1.5, 2.5):
        for k in range(6):
            s = corners[k].sum(1) - c
            m = int(((s < 0) << np.arange(4)).sum())
            for tri in M.case_triangles(k, m):
                p = [corners[k][u] + (s[u] / (s[u] - s[v])) * (corners[k][v] - corners[k][u]) for u, v in tri]
                n = np.cross(p[1] - p[0], p[2] - p[0])
                assert n.sum() > 0, (c, k, m)


def test_ply_round_trip(tmp_path):
    """write_ply (the library's host-only writer) then read_ply reproduces the triangle list exactly;
    the vertex count is the number of distinct vertices."""
    from topfusion_amd import io
    for name, tris in (("sphere", M.sphere_case()[2]), ("random", M.random_case()[2]), ("empty", np.zeros((0, 3, 3), np.float32))):
        path = tmp_path / f"{name}.ply"
        io.write_ply(path, tris)
        verts, faces = io.read_ply(path)
        assert faces.shape == (len(tris), 3)
        got = verts[faces] if len(tris) else np.zeros((0, 3, 3), np.float32)
        assert np.array_equal(got.view(np.uint32), np.asarray(tris).view(np.uint32)), name
        distinct = len(np.unique(np.asarray(tris).reshape(-1, 3).view(np.uint32), axis=0)) if len(tris) else 0
        assert len(verts) == distinct, (name, len(verts), distinct)
