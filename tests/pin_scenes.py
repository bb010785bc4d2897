"""The scenes and inputs of the reference stage pin (oracle/ref_pin/ref_pin_stages.cpp), in one
language only: tests/golden/make_golden.py feeds them to the reference's own per-element functions,
tests/test_oracle_stage_pin.py and tests/test_gpu_stage_pin.py feed the same arrays to the oracle
and to the HIP kernels.  Every golden records the CRC32 of the scene's hash and VBA bytes.

Everything is made from integers: lowbias32 hashing (synth._mix32, no np.random), integer
distances, rational rotations (integer quaternions) and millimetre / 1/64-voxel coordinates, each
rounded to float32 once.

Hash tables have the reference's compile-time sizes (VoxelBlockHash.hpp:14-18; the hash mask is
compiled into hashIndex): 0x100000 buckets, 0x20000 excess entries; at most 0x1000 voxel blocks.

  pin file: b"TFPIN1\\0\\0", u32 n, then n arrays: name[24] (NUL padded), u32 type code
  (0 u8, 1 i16, 2 i32, 3 u32, 4 f32), u32 element count, the elements (little endian), padded to
  a multiple of 4 bytes.
"""
import itertools
import os
import zlib

import numpy as np

from topfusion_amd import synth
from vbh_ref import HASH_DTYPE, VOXEL_DTYPE, chain

N_BUCKETS, N_EXCESS, N_BLOCKS = 0x100000, 0x20000, 0x1000
N_TOTAL = N_BUCKETS + N_EXCESS
W, H = 96, 72
SCENES = ("sphere", "random", "plane")
CASES = ("sdf_read", "raycast", "integrate", "alloc_pp", "visibility", "expected_depths", "pixels")

FAR_AWAY, VERY_CLOSE = np.float32(999999.9), np.float32(0.05)     # VisualisationEngine_Shared.hpp:17-23
MU, MAXW, VOXEL_SIZE, VF_MIN, VF_MAX = np.float32(0.02), 100, np.float32(0.005), np.float32(0.2), np.float32(3.0)

MAX_GOLDEN_BYTES = 360476     # no stage pin golden larger than the largest of the first six (ref_pin_colour.bin)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- pin files ------------------------------------------------------------------------------------
_MAGIC = b"TFPIN1\0\0"
_TYPES = (np.dtype("u1"), np.dtype("<i2"), np.dtype("<i4"), np.dtype("<u4"), np.dtype("<f4"))


def write_pin(path, arrays):
    with open(path, "wb") as f:
        f.write(_MAGIC)
        f.write(np.uint32(len(arrays)).tobytes())
        for name, a in arrays.items():
            a = np.ascontiguousarray(a)
            code = _TYPES.index(a.dtype)
            nm = name.encode()
            assert len(nm) < 24, name
            f.write(nm.ljust(24, b"\0"))
            f.write(np.array([code, a.size], "<u4").tobytes())
            b = a.tobytes()
            f.write(b + b"\0" * (-len(b) % 4))


def read_pin(path):
    with open(path, "rb") as f:
        buf = f.read()
    assert buf[:8] == _MAGIC, path
    n = int(np.frombuffer(buf, "<u4", 1, 8)[0])
    off, out = 12, {}
    for _ in range(n):
        name = buf[off:off + 24].rstrip(b"\0").decode()
        code, count = (int(v) for v in np.frombuffer(buf, "<u4", 2, off + 24))
        dt = _TYPES[code]
        off += 32
        out[name] = np.frombuffer(buf, dt, count, off)
        off += (count * dt.itemsize + 3) & ~3
    assert off == len(buf), path
    return out


def golden_path(scene, case):
    return os.path.join(GOLDEN, f"stage_pin_{scene}_{case}.bin")


# ---- integer randomness -----------------------------------------------------------------------------
def _h(seed, *keys):
    """uint32 hash of integer arrays (lowbias32 chained over the keys)."""
    h = np.uint32(seed)
    for k in keys:
        h = synth._mix32((np.asarray(h, np.uint64) + (np.asarray(k, np.int64) & 0xFFFFFFFF).astype(np.uint64)
                          + np.uint64(0x9E3779B9)).astype(np.uint64) & np.uint64(0xFFFFFFFF))
    return np.asarray(h, np.uint32)


def _isqrt(n):
    """floor(sqrt(n)) of an int64 array (n < 2^52), exactly."""
    s = np.floor(np.sqrt(n.astype(np.float64))).astype(np.int64)
    s -= s * s > n
    s += (s + 1) * (s + 1) <= n
    return s


# ---- poses ------------------------------------------------------------------------------------------
def _rotation(q):
    """The rotation of the integer quaternion (w, x, y, z): rational entries, float64."""
    w, x, y, z = (int(v) for v in q)
    n = w * w + x * x + y * y + z * z
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]], np.float64) / n


def camera(q, centre_um):
    """(camera-to-world, world-to-camera) [R|t] 3x4 float32 of a camera at centre_um (micrometres)
    with the rotation of the integer quaternion q."""
    R = _rotation(q)
    c = np.asarray(centre_um, np.float64) / 1e6
    c2w = np.concatenate([R, c[:, None]], 1).astype(np.float32)
    w2c = np.concatenate([R.T, (-R.T @ c)[:, None]], 1).astype(np.float32)
    return c2w, w2c


def _edge_translation(target, f, c0, z0, nominal):
    """A float32 translation t for which a voxel coordinate p = n * voxelSize projects exactly onto
    `target`: RN(RN(RN(f * RN(p + t)) / z0) + c0) == target, and the same with (f x) * (1 / z0) in place
    of the division (the two forms the reference's host build and its CUDA build compute), searched
    over the floats around the real solution, with the camera near `nominal`."""
    f, c0, z0 = np.float32(f), np.float32(c0), np.float32(z0)
    xc = (float(target) - float(c0)) / float(f) * float(z0)
    n0 = int(round((nominal + xc) / float(VOXEL_SIZE)))
    for n in (n0, n0 - 1, n0 + 1, n0 - 2, n0 + 2, n0 - 3, n0 + 3):
        p = np.float32(n) * VOXEL_SIZE
        ts = (np.float32(xc - float(p)).view(np.int32) + np.arange(-60000, 60001, dtype=np.int32)).view(np.float32)
        fxp = (f * (p + ts).astype(np.float32)).astype(np.float32)
        ok = np.nonzero(((fxp / z0).astype(np.float32) + c0 == np.float32(target))
                        & ((fxp * (np.float32(1) / z0)).astype(np.float32) + c0 == np.float32(target)))[0]
        if len(ok):
            return ts[ok[len(ok) // 2]]
    raise AssertionError("no translation puts a voxel on the edge")


def edge_camera(nominal_um, plane, x_target, y_target):
    """An axis-aligned camera near nominal_um (micrometres), behind the voxel plane z = `plane` by
    nominal_um's distance, placed so that one voxel column projects exactly to pt_image.x == x_target and
    one voxel row exactly to pt_image.y == y_target."""
    fx, fy, cx, cy = intrinsics()
    for back_um in range(0, 4000, 100):             # (not every z0 has a float v with RN(v / z0) on the edge: step back until one has)
        tz = np.float32(-(nominal_um[2] - back_um) / 1e6)
        z0 = np.float32(np.float32(plane) * VOXEL_SIZE + tz)
        try:
            t = np.array([_edge_translation(x_target, fx, cx, z0, nominal_um[0] / 1e6),
                          _edge_translation(y_target, fy, cy, z0, nominal_um[1] / 1e6), tz], np.float32)
            break
        except AssertionError:
            continue
    w2c = np.concatenate([np.eye(3, dtype=np.float32), t[:, None]], 1)
    c2w = np.concatenate([np.eye(3, dtype=np.float32), -t[:, None]], 1)
    return c2w, w2c


def intrinsics():
    return tuple(np.float32(v) for v in synth.intrinsics(W, H))


# ---- scenes -----------------------------------------------------------------------------------------
_LOCAL = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")[::-1], -1).reshape(512, 3)  # x + 8y + 64z


def _colours(n):
    i = np.arange(n, dtype=np.int64)
    rgb = _h(61, i) & np.uint32(0xFFFFFF)
    wc = np.array([0, 1, 5, 100], np.uint32)[_h(62, i) % np.uint32(4)]
    return (rgb | (wc << np.uint32(24))).astype(np.uint32)


SPHERE_C16 = (54, -42, 2244)            # centre in 1/16 voxel: (3.375, -2.625, 140.25) voxels
SPHERE_RQ = 56 * 256 + 80               # radius in 1/256 voxel
SPHERE_BAND = 4 * 256                   # mu in 1/256 voxel


def _sphere():
    """A sphere of radius 56.3 voxels about (3.375, -2.625, 140.25): its surface straddles negative x
    and y block coordinates.  sdf = clamp((d - r) / mu) from the integer distance d (1/256 voxel), in
    every block the band |d - r| <= mu touches; w from {1, 5, 100}; about one block in 30 swapped out."""
    cb = np.array([0, -1, 17])
    blocks = np.array(list(itertools.product(range(-9, 10), repeat=3)), np.int64)[:, ::-1] + cb
    vox = blocks[:, None, :] * 8 + _LOCAL[None]                       # (n, 512, 3)
    d2 = ((16 * vox - np.array(SPHERE_C16)) ** 2).sum(-1)
    dq = _isqrt(d2 * 256) - SPHERE_RQ
    keep = (np.abs(dq) <= SPHERE_BAND).any(1)
    blocks, vox, dq = blocks[keep], vox[keep], dq[keep]
    assert len(blocks) <= N_BLOCKS, len(blocks)
    h, entry, last_excess = synth.build_hash(blocks, N_BUCKETS, N_EXCESS, HASH_DTYPE)
    # every 30th block or so swapped out (ptr -1), none around cameras b and c
    out = (_h(12, blocks[:, 0], blocks[:, 1], blocks[:, 2]) % np.uint32(30) == 0) & (np.abs(blocks - np.array([0, -1, 10])).max(1) > 2)
    h["ptr"][entry[out]] = -1
    vba = np.zeros(N_BLOCKS * 512, VOXEL_DTYPE)
    vba["sdf"] = 32767
    n = len(blocks) * 512
    vba["sdf"][:n] = np.clip((dq * 32767) // SPHERE_BAND, -32767, 32767).reshape(-1)
    vba["w"][:n] = np.array([1, 5, 100], np.uint8)[_h(11, vox[..., 0], vox[..., 1], vox[..., 2]).reshape(-1) % np.uint32(3)]
    rgb = np.zeros(N_BLOCKS * 512, np.uint32)
    rgb[:n] = _colours(n)
    return dict(hash=h, vba=vba, vba_rgb=rgb, blocks=blocks, entry=entry, last_excess=last_excess,
                special=np.zeros((0, 3), np.int64),
                cam_a=camera((40, 1, -2, 1), (13000, -7000, 2000)),
                # on the near side of the shell, inside allocated space
                cam_b=camera((10, 1, 2, 0), (16200, -14300, 418000)),
                # 6 cm further in: the image plane cuts the shell in a circle of blocks on every side
                cam_d=camera((40, 1, -2, 1), (16200, -14300, 478000)),
                # axis-aligned, 6 voxels behind the voxel plane z = 84 (see integrate_inputs)
                cam_c=edge_camera((16200, -14300, 390000), 84, 1, H - 2),
                cam_e=edge_camera((16200, -14300, 390000), 84, W - 2, 1))


PLANE_N, PLANE_P0 = (2, 3, 6), (2, -3, 150)     # normal (length 7) and a point of the slab, voxels


def _plane():
    """A slab seen obliquely: the plane through (2, -3, 150) with normal (2, 3, 6) / 7, 21 x 17 blocks wide
    across negative and positive x and y.  sdf = clamp(s / mu) from the integer signed distance s = -n . (p - p0)
    (1/7 voxel), in every block with a voxel from mu in front of the surface to 44 voxels behind it (the slab is 22 cm thick); w from {1, 5, 100}; about one block in 30 swapped out."""
    blocks = np.array(list(itertools.product(range(-10, 11), range(-8, 9), range(8, 36))), np.int64)
    vox = blocks[:, None, :] * 8 + _LOCAL[None]
    sd = -((vox - np.array(PLANE_P0)) * np.array(PLANE_N)).sum(-1)           # positive on the cameras' side
    keep = ((sd <= 4 * 7) & (sd >= -44 * 7)).any(1)
    blocks, vox, sd = blocks[keep], vox[keep], sd[keep]
    assert len(blocks) <= N_BLOCKS, len(blocks)
    h, entry, last_excess = synth.build_hash(blocks, N_BUCKETS, N_EXCESS, HASH_DTYPE)
    out = (_h(13, blocks[:, 0], blocks[:, 1], blocks[:, 2]) % np.uint32(30) == 0) & (np.abs(blocks - np.array([0, -1, 18])).max(1) > 2)
    h["ptr"][entry[out]] = -1
    vba = np.zeros(N_BLOCKS * 512, VOXEL_DTYPE)
    vba["sdf"] = 32767
    n = len(blocks) * 512
    vba["sdf"][:n] = np.clip((sd * 32767) // (4 * 7), -32767, 32767).reshape(-1)
    vba["w"][:n] = np.array([1, 5, 100], np.uint8)[_h(14, vox[..., 0], vox[..., 1], vox[..., 2]).reshape(-1) % np.uint32(3)]
    rgb = np.zeros(N_BLOCKS * 512, np.uint32)
    rgb[:n] = _colours(n)
    return dict(hash=h, vba=vba, vba_rgb=rgb, blocks=blocks, entry=entry, last_excess=last_excess,
                special=np.zeros((0, 3), np.int64),
                cam_a=camera((40, 1, -2, 1), (5000, -9000, 100000)),
                cam_b=camera((8, 5, 0, 0), (7150, -19300, 741400)),            # 2 voxels in front of the surface (allocated), looking along it
                cam_c=edge_camera((10300, -15200, 720000), 150, 1, H - 2),     # 6 voxels behind the voxel plane z = 150
                cam_e=edge_camera((10300, -15200, 720000), 150, W - 2, 1),
                cam_d=camera((40, 1, -2, 1), (10300, -15200, 765000)))         # its image plane cuts the slab


def _collision_groups(lo, hi, size, count, avoid):
    """`count` groups of `size` block positions in the box [lo, hi) that share one hashIndex under
    the 2^20 mask (brute force over the box), none of them in `avoid`."""
    ax = [np.arange(lo[k], hi[k], dtype=np.int64) for k in range(3)]
    pos = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    hi_ = synth.hash_index(pos[:, 0], pos[:, 1], pos[:, 2], N_BUCKETS)
    order = np.argsort(hi_, kind="stable")
    hs = hi_[order]
    start = np.nonzero(np.r_[True, hs[1:] != hs[:-1]])[0]
    length = np.diff(np.r_[start, len(hs)])
    groups = []
    for s in start[length >= size]:
        g = pos[order[s:s + size]]
        if not any(tuple(p) in avoid for p in g.tolist()):
            groups.append(g)
    groups.sort(key=lambda g: (int(np.abs(g[:, :2]).max() + g[:, 2].max() // 2), g.tolist()))     # the nearest to the view axis
    groups = groups[:count]
    assert len(groups) == count, len(groups)
    return groups


def _random():
    """~60 % of the blocks of a 12 x 10 x 11 box in front of the camera (negative x and y included),
    plus 12 groups of 4 positions sharing one hashIndex (bucket entry + an excess chain of 3): some
    chain members swapped out (ptr -1), one unallocated in mid-chain (ptr -2).  VBA pointers shuffled;
    sdf over the whole short range with 0 and +-32767 frequent; w from {0, 1, 5, 100}."""
    box = np.array(list(itertools.product(range(-6, 6), range(-5, 5), range(12, 23))), np.int64)
    forced = (np.abs(box - np.array([0, -1, 17])).sum(1) <= 1) | (np.abs(box - np.array([0, -1, 16])).sum(1) == 0)
    box = box[(_h(21, box[:, 0], box[:, 1], box[:, 2]) % np.uint32(10) < 6) | forced]      # the blocks around cameras b and c always
    avoid = {tuple(p) for p in box.tolist()}
    groups = _collision_groups((-40, -40, 4), (40, 40, 60), 4, 12, avoid)
    special = np.concatenate(groups)
    blocks = np.concatenate([box, special])
    assert len(blocks) <= N_BLOCKS
    h, entry, last_excess = synth.build_hash(blocks, N_BUCKETS, N_EXCESS, HASH_DTYPE)
    perm = np.argsort(_h(22, np.arange(N_BLOCKS)), kind="stable")[:len(blocks)]
    h["ptr"][entry] = perm
    nb = len(box)
    out = (_h(25, box[:, 0], box[:, 1], box[:, 2]) % np.uint32(25) == 0) & (np.abs(box - np.array([0, -1, 16])).max(1) > 2)
    h["ptr"][entry[:nb][out]] = -1                                       # every 25th box block or so swapped out
    chains = [entry[nb + 4 * g: nb + 4 * g + 4] for g in range(len(groups))]
    for g, ch in enumerate(chains):
        assert ch[0] < N_BUCKETS and np.all(ch[1:] >= N_BUCKETS)         # bucket entry, then three excess entries
        walk = list(chain(h, N_BUCKETS, groups[g][0]))
        assert len(walk) == 4 and walk[0] == ch[0]
        if g % 3 == 0:
            h["ptr"][walk[1]] = -1                                       # swapped out, mid-chain
        if g % 3 == 1:
            h["ptr"][walk[3]] = -1                                       # swapped out, chain end
        if g == 2:
            h["ptr"][walk[2]] = -2                                       # unallocated, mid-chain
        if g == 5:
            h["ptr"][walk[0]] = -1                                       # the bucket entry itself swapped out
    i = np.arange(N_BLOCKS * 512, dtype=np.int64)
    vba = np.zeros(N_BLOCKS * 512, VOXEL_DTYPE)
    r = _h(23, i)
    sdf = (r >> np.uint32(16)).astype(np.int64) - 32768
    pick = r & np.uint32(0xFF)
    sdf[pick < 20] = 0
    sdf[(pick >= 20) & (pick < 36)] = 32767
    sdf[(pick >= 36) & (pick < 52)] = -32767
    vba["sdf"] = sdf
    vba["w"] = np.array([0, 1, 5, 100], np.uint8)[_h(24, i) % np.uint32(4)]
    return dict(hash=h, vba=vba, vba_rgb=_colours(N_BLOCKS * 512), blocks=blocks, entry=entry, last_excess=last_excess,
                special=special,
                cam_a=camera((40, -1, 2, 1), (-9000, 6000, 3000)),
                cam_b=camera((10, 2, -1, 1), (21000, -12000, 662500)),     # inside the box
                cam_d=camera((10, 1, 10, 0), (21000, -12000, 662500)),
                cam_c=edge_camera((21000, -12000, 650000), 136, 1, H - 2),   # 6 voxels behind the voxel plane z = 136
                cam_e=edge_camera((21000, -12000, 650000), 136, W - 2, 1))


_cache = {}


def scene(name):
    """The scene `name`: dict of hash, vba, vba_rgb (read-only), block positions, their entry indices,
    lastFreeExcessListId, the collision-group positions and the cameras."""
    if name not in _cache:
        s = {"sphere": _sphere, "random": _random, "plane": _plane}[name]()
        for k in ("hash", "vba", "vba_rgb", "blocks", "entry", "special"):
            s[k].setflags(write=False)
        s["crc"] = np.array([zlib.crc32(s["hash"].tobytes()), zlib.crc32(s["vba"].tobytes()),
                             zlib.crc32(s["vba_rgb"].tobytes())], np.uint32)
        _cache[name] = s
    return _cache[name]


# ---- inputs of the cases ----------------------------------------------------------------------------
def range_image(name):
    """The supplied rendering range image, (H, W, 2) float32; castRay reads cell (x / 8, y / 8) with the
    row stride W (genericRaycast_device's locId2).  Most cells hold the frustum; a hashed third of
    them a narrower range, min == max, min > max or the FAR_AWAY / VERY_CLOSE initial pair."""
    r = np.empty((H, W, 2), np.float32)
    r[..., 0], r[..., 1] = VF_MIN, VF_MAX
    seed = 31 + SCENES.index(name)
    for cy in range(H // 8):
        for cx in range(W // 8):
            k = int(_h(seed, cx, cy) % np.uint32(12))
            if k == 0:
                r[cy, cx] = (FAR_AWAY, VERY_CLOSE)
            elif k == 1:
                r[cy, cx] = (0.7, 0.7)
            elif k == 2:
                r[cy, cx] = (1.0, 0.5)
            elif k == 3:
                r[cy, cx] = (0.45, 1.25)
    return r


def sdf_points(name, n=4096):
    """n read positions (voxel units, float32; every coordinate a multiple of 1/64, so exact): in
    runs of four per block (the carried IndexCache hits and misses), at exact integers, half-integers,
    other fractions, block faces and corners whose +1 neighbours lie in the next block (present,
    missing, swapped out or chained), just below a block's origin, and in unallocated space."""
    s = scene(name)
    blocks = np.concatenate([s["special"], s["blocks"]]) if len(s["special"]) else s["blocks"]
    i = np.arange(n, dtype=np.int64)
    run = i // 4
    nsp = len(s["special"]) if len(s["special"]) else len(blocks)        # every third run in a collision-group block
    b = blocks[np.where(run % 3 == 0, _h(41, run) % np.uint32(nsp), _h(42, run) % np.uint32(len(blocks)))]
    kind = _h(43, i) % np.uint32(8)
    loc = np.stack([_h(44 + k, i) % np.uint32(8 * 64) for k in range(3)], -1).astype(np.int64)     # 1/64 voxel inside the block
    loc = np.where((kind == 0)[:, None], loc // 64 * 64, loc)                                      # exact integers
    loc = np.where((kind == 1)[:, None], loc // 64 * 64 + 32, loc)                                 # half-integers
    face = 7 * 64 + (loc % 64)
    ax = (_h(47, i) % np.uint32(3)).astype(np.int64)
    onax = np.arange(3)[None] == ax[:, None]
    loc = np.where((kind == 3)[:, None] & onax, face, loc)                                         # one +face
    loc = np.where((kind == 4)[:, None], face, loc)                                                # the +++ corner
    loc = np.where((kind == 5)[:, None] & onax, -(loc % 64) - 1, loc)                              # just below the origin
    loc = np.where((kind == 6)[:, None], loc + 8 * 64 * np.array([1, -1, 1]), loc)                 # a diagonal neighbour block
    loc = np.where((kind == 7)[:, None] & onax, 7 * 64, loc)                                       # exactly on the last voxel plane
    p64 = b * 8 * 64 + loc
    return (p64.astype(np.float64) / 64).astype(np.float32)


def visibility_blocks(name, n=4096):
    """n block positions around the frustum of camera b: behind the camera, across every image edge
    and in the enlarged border of an eighth of the image."""
    i = np.arange(n, dtype=np.int64)
    seed = 51 + SCENES.index(name)
    c = np.asarray(scene(name)["cam_b"][0][:, 3], np.float64) / 0.04
    lo, span = np.floor(c).astype(np.int64) - np.array([14, 12, 10]), np.array([28, 24, 24])
    return (lo + np.stack([_h(seed + 10 * k, i) % np.uint32(span[k]) for k in range(3)], -1)).astype(np.int16)


def rgb_image(name):
    i = np.arange(W * H, dtype=np.int64)
    return _h(71 + SCENES.index(name), i).view(np.uint8).reshape(H, W, 4).copy()


def integrate_inputs(name):
    """Three frames, each applied to the scene as it is: (world-to-camera pose, dists image, visible
    list).  Frame 0: camera b (inside allocated space, so listed blocks lie behind it too) and
    8 x 8 pixel tiles of hashed depths: 0, negative, 3 m (eta / mu > 1) and 1 .. 51 cm, where the listed blocks lie.
    Frames 1 and 2: cameras c and e, axis-aligned, 6 voxels behind a voxel plane, and placed (edge_camera) so
    that a voxel column and a voxel row project exactly onto pt_image.x == 1 / W - 2 and pt_image.y == H - 2 / 1,
    the edges of the update's window; the plane's voxels have
    pt_camera.z = z0 in [2^-6, 2^-5): the image holds z0 - mu, exact in float32, so eta == -mu to
    the bit there.  The list holds every 12th allocated entry, the entries of the blocks around
    the cameras, an unallocated entry (ptr -2) and, where the scene has them, swapped-out ones."""
    s = scene(name)
    seed = 81 + SCENES.index(name)
    h = s["hash"]
    live = np.nonzero(h["ptr"] >= 0)[0]
    near = []
    for cam in ("cam_b", "cam_c", "cam_e"):
        cb = np.floor(np.asarray(s[cam][0][:, 3], np.float64) / 0.04).astype(np.int64)
        d = np.abs(np.stack([h["x"][live], h["y"][live], h["z"][live]], -1).astype(np.int64) - cb).max(1)
        near.append(live[d <= 1])
    empty = np.nonzero(h["ptr"][:N_BUCKETS] < -1)[0][:1]
    swapped = np.nonzero(h["ptr"] == -1)[0]
    vis = np.unique(np.concatenate([live[::12], *near, empty, swapped])).astype(np.int32)
    ty, tx = np.meshgrid(np.arange(H) // 8, np.arange(W) // 8, indexing="ij")
    k = _h(seed, tx, ty) % np.uint32(16)
    r = _h(seed + 1, tx, ty)
    mm = 10 + np.where(r & np.uint32(1), (r >> np.uint32(1)) % np.uint32(110), (r >> np.uint32(1)) % np.uint32(500)).astype(np.int64)
    d0 = (mm.astype(np.float32) / np.float32(1000)).astype(np.float32)
    d0[k == 0] = 0.0
    d0[k == 1] = -0.5
    d0[k == 2] = 3.0
    # frames 1 and 2: z0 = RN(plane + t_z) as Matrix4f * Vector4f forms it for an axis-aligned pose
    frames = [(s["cam_b"][1], d0, vis)]
    for k, cam in enumerate(("cam_c", "cam_e")):
        w2c = s[cam][1]
        plane = np.float32({"sphere": 84, "random": 136, "plane": 150}[name]) * VOXEL_SIZE
        z0 = np.float32(plane + w2c[2, 3])
        assert np.float32(2.0 ** -6) <= z0 < np.float32(2.0 ** -5) and z0 > MU
        near_d = np.float32(z0 - MU)
        assert np.float32(near_d - z0) == -MU and near_d > 0
        d1 = np.full((H, W), near_d, np.float32)
        sel = (_h(seed + 2 + k, tx, ty) % np.uint32(5) == 0) & (tx > 0) & (tx < W // 8 - 1) & (ty > 0) & (ty < H // 8 - 1)
        d1[sel] = d0[sel]
        frames.append((w2c, d1, vis))
    return frames


def expected_depths_list(name):
    """The visible list of the expected-depths case, seen from camera d (inside allocated space:
    blocks with corners behind the camera, huge projections clamped at every image side, rejected
    ones): every allocated entry, the swapped-out ones and an unallocated one, by entry index."""
    h = scene(name)["hash"]
    return np.unique(np.concatenate([np.nonzero(h["ptr"] >= -1)[0], np.nonzero(h["ptr"][:N_BUCKETS] < -1)[0][:1]])).astype(np.int32)


ALLOC_DROP = {"sphere": (), "random": (4375,), "plane": ()}      # pixels (x + y * W) whose requests collide with another pixel's: found by the pin program


def alloc_inputs(name):
    """(world-to-camera pose of camera a, dists image) of the allocation case.  Most pixels hold 0; the
    others are aimed (the aim needs no precision: it only chooses inputs) at allocated blocks,
    swapped-out blocks, blocks chained in excess entries, unallocated positions whose bucket is taken
    (requests of type 2) and free positions (type 1); a few hold negative depths and a millimetre
    either side of both frustum limits (d - mu against viewFrustum_min, d + mu against
    viewFrustum_max).  Requests are kept sparse because two requested blocks that share a bucket make
    the reference's arrays depend on the pixel order; the pixels of ALLOC_DROP are set to 0 for that."""
    s = scene(name)
    seed = 91 + SCENES.index(name)
    c2w, w2c = s["cam_a"]
    h = s["hash"]
    fx, fy, cx, cy = (float(v) for v in intrinsics())
    d = np.zeros((H, W), np.float32)
    idx = np.arange(N_TOTAL)
    live, swapped = np.nonzero(h["ptr"] >= 0)[0], np.nonzero(h["ptr"] == -1)[0]
    taken = set(zip(h["x"][h["ptr"] >= -1].tolist(), h["y"][h["ptr"] >= -1].tolist(), h["z"][h["ptr"] >= -1].tolist()))
    ax = [np.arange(-12, 12), np.arange(-9, 9), np.arange(8, 30)]
    cand = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3)
    cand = cand[[tuple(p) not in taken for p in cand.tolist()]]
    occupied = h["ptr"][synth.hash_index(cand[:, 0], cand[:, 1], cand[:, 2], N_BUCKETS)] >= -1
    pick = lambda a, n, k: a[np.argsort(_h(seed + k, np.arange(len(a))), kind="stable")[:n]]
    ent = lambda e: np.stack([h["x"][e], h["y"][e], h["z"][e]], -1).astype(np.int64)
    targets = np.concatenate([ent(pick(live[live < N_BUCKETS], 60, 1)), ent(pick(live[live >= N_BUCKETS], 40, 2)), ent(pick(swapped, 40, 3)),
                              pick(cand[occupied], 60, 4), pick(cand[~occupied], 40, 5)])
    pc = (targets + 0.5) * 0.04 @ w2c[:, :3].astype(np.float64).T + w2c[:, 3].astype(np.float64)
    for x, y, z in pc[pc[:, 2] > 0.25]:
        u, v = int(round(fx * x / z + cx)), int(round(fy * y / z + cy))
        if 0 <= u < W and 0 <= v < H:
            d[v, u] = np.float32(int(round(z * 1000))) / np.float32(1000)
    # the gates: 0 stays 0; negative; d - mu = 0.199, 0.200, 0.201; d + mu = 2.999, 3.000, 3.001
    for k in range(96):
        mm = (219, 2981, 219, 2981, -300, (220, 221, 2979, 2980)[k // 6 % 4])[k % 6]
        d[36 + 3 * (k % 12), k] = np.float32(mm) / np.float32(1000)
    d.reshape(-1)[list(ALLOC_DROP[name])] = 0
    return w2c, d


def pin_inputs(name):
    """Everything oracle/ref_pin/ref_pin_stages.cpp reads for one scene, as a pin file's arrays."""
    s = scene(name)
    fx, fy, cx, cy = intrinsics()
    fr = integrate_inputs(name)
    return {
        "hash": s["hash"].view(np.uint8), "vba": s["vba"].view(np.uint8), "vba_rgb": s["vba_rgb"], "crc": s["crc"],
        "fparams": np.array([fx, fy, cx, cy, MU, VOXEL_SIZE, VF_MIN, VF_MAX], np.float32),
        "iparams": np.array([W, H, MAXW], np.int32),
        "c2w_a": s["cam_a"][0].reshape(12), "c2w_b": s["cam_b"][0].reshape(12), "w2c_b": s["cam_b"][1].reshape(12),
        "w2c_d": s["cam_d"][1].reshape(12),
        "range": range_image(name).reshape(-1),
        "sdf_points": sdf_points(name).reshape(-1),
        "vis_blocks": visibility_blocks(name).reshape(-1),
        "rgb": rgb_image(name).reshape(-1), "ed_vis": expected_depths_list(name),
        "alloc_pose": alloc_inputs(name)[0].reshape(12), "alloc_dists": alloc_inputs(name)[1].reshape(-1),
        **{f"int_{key}{k}": v.reshape(-1) for k, f in enumerate(fr) for key, v in zip(("pose", "dists", "vis"), f)},
    }


# ---- coverage conditions ------------------------------------------------------------------------------
MIN_HITS = 16


def check_coverage(case, d):
    """The conditions a golden must meet (asserted when it is written and again by the CPU test):
    every branch the pin program counts is hit at least MIN_HITS times; 25 % .. 90 % of the rays of
    each raycast are found."""
    c = np.asarray(d["counts"], np.int64)
    if case == "raycast":
        for found, missed, degenerate, marked, missing_steps, interpolated in c.reshape(2, 6):
            assert min(found, missed, degenerate, marked, missing_steps, interpolated) >= MIN_HITS, c
            assert 0.25 <= found / (W * H) <= 0.90, c
    elif case == "integrate":
        t = c.reshape(3, 12).sum(0)
        assert t[0] >= 1, c                          # a list entry with ptr < 0
        assert t[1:11].min() >= MIN_HITS, c
        assert c.reshape(3, 12)[1:, 11].min() >= 1, c    # updated voxels with pt_image exactly on the window's edge, frames 1 and 2
    elif case == "alloc_pp":
        assert c[:10].min() >= MIN_HITS, c          # (c[10], pixels with noSteps == 1, is recorded only)
    elif case == "expected_depths":
        assert c[0] >= 1 and c[1:].min() >= MIN_HITS, c
    elif case == "pixels":
        assert c.min() >= MIN_HITS and W * H - c[:6].max() >= MIN_HITS, c  # lit and unlit pixels in every image, both doPlus1 branches
    else:
        assert c.min() >= MIN_HITS, c
