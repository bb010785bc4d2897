"""Frame files of the reference demo (apps/demo.cpp:91-97): 16-bit PGM depth + 8-bit PPM colour.

Same pixels as OpenCV's imread(path, CV_16U) / imread(path) for binary netpbm files: P5 with
maxval > 255 holds big-endian 16-bit samples; P6 holds RGB, returned as BGR like imread.
The C++ side is include/tfusion/io.hpp (readPGM16 / readPPM / FrameSequenceSource).

Mesh output (an addition): write_ply / write_ply_indexed / read_ply, the binary PLY of tf_mesh_write_ply."""
import numpy as np


def _header(buf, magic):
    if buf[:2] != magic:
        raise ValueError(f"not a binary {magic.decode()} file")
    fields, i = [], 2
    while len(fields) < 3:
        while buf[i:i + 1] in (b" ", b"\t", b"\r", b"\n") or buf[i:i + 1] == b"#":
            if buf[i:i + 1] == b"#":
                while buf[i:i + 1] not in (b"\n", b""):
                    i += 1
            i += 1
        j = i
        while buf[j:j + 1].isdigit():
            j += 1
        if j == i:
            raise ValueError("bad netpbm header")
        fields.append(int(buf[i:j]))
        i = j
    return fields, i + 1            # one whitespace byte ends the header


def read_pgm16(path):
    """(rows, cols) uint16 depth of a P5 PGM."""
    buf = open(path, "rb").read()
    (cols, rows, maxval), off = _header(buf, b"P5")
    if maxval > 255:
        return np.frombuffer(buf, ">u2", cols * rows, off).reshape(rows, cols).astype(np.uint16)
    return np.frombuffer(buf, np.uint8, cols * rows, off).reshape(rows, cols).astype(np.uint16)


def write_pgm16(path, depth):
    d = np.ascontiguousarray(depth, np.uint16)
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n65535\n" % (d.shape[1], d.shape[0]))
        f.write(d.astype(">u2").tobytes())


def read_ppm(path):
    """(rows, cols, 3) uint8 B, G, R of a P6 PPM."""
    buf = open(path, "rb").read()
    (cols, rows, maxval), off = _header(buf, b"P6")
    if maxval > 255:
        raise ValueError("16-bit PPM not supported")
    rgb = np.frombuffer(buf, np.uint8, cols * rows * 3, off).reshape(rows, cols, 3)
    return rgb[..., ::-1].copy()


def write_ppm(path, bgr):
    b = np.ascontiguousarray(bgr, np.uint8)
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (b.shape[1], b.shape[0]))
        f.write(b[..., ::-1].tobytes())


def read_sequence(depth_pattern, first=0, count=None):
    """Frames depth_pattern % i for i = first, first+1, ... until the first missing file."""
    import os
    out, i = [], first
    while (count is None or len(out) < count) and os.path.exists(depth_pattern % i):
        out.append(read_pgm16(depth_pattern % i))
        i += 1
    return np.stack(out) if out else np.zeros((0, 0, 0), np.uint16)


def write_ply(path, tris, normals=None, colours=None):
    """Triangles (n, 3, 3) float32 as a binary little-endian PLY, vertices welded by exact bit
    equality (tf_mesh_write_ply, the writer TopFu.save_mesh uses).  normals (n, 3, 3) float32 and
    colours (n, 3, 4) uint8 RGBA, when given, become the vertex properties nx ny nz and red green blue
    alpha, and vertices weld on the whole record (tf_mesh_write_ply_attr)."""
    import ctypes
    from . import _lib as L
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3, 3)
    if normals is None and colours is None:
        L.check(L.load().tf_mesh_write_ply(str(path).encode(), t.ctypes.data_as(ctypes.c_void_p), len(t)), "tf_mesh_write_ply")
        return
    nr = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3, 3)
    co = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 3, 4)
    for a in (nr, co):
        if a is not None and len(a) != len(t):
            raise ValueError("attributes and triangles differ in length")
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    L.check(L.load().tf_mesh_write_ply_attr(str(path).encode(), vp(t), vp(nr), vp(co), len(t)), "tf_mesh_write_ply_attr")


def write_ply_indexed(path, vertices, indices, normals=None, colours=None):
    """An indexed mesh -- vertices (m, 3) float32, indices (n, 3) uint32, optionally normals (m, 3) float32 and
    colours (m, 4) uint8 RGBA per vertex -- as a binary little-endian PLY with write_ply's layout: the vertex
    table as given, nothing welded (tf_mesh_write_ply_indexed).  read_ply / read_ply_attr read it."""
    import ctypes
    from . import _lib as L
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    f = np.ascontiguousarray(indices, np.uint32).reshape(-1, 3)
    nr = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    co = None if colours is None else np.ascontiguousarray(colours, np.uint8).reshape(-1, 4)
    for a in (nr, co):
        if a is not None and len(a) != len(v):
            raise ValueError("attributes and vertices differ in length")
    vp = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(ctypes.c_void_p)
    dummy = np.zeros(4, np.float32)           # an empty attribute column is still declared
    at = lambda a: None if a is None else (vp(a) or dummy.ctypes.data_as(ctypes.c_void_p))
    L.check(L.load().tf_mesh_write_ply_indexed(str(path).encode(), vp(v), at(nr), at(co), len(v), vp(f), len(f)),
            "tf_mesh_write_ply_indexed")


def read_ply(path):
    """(vertices (m, 3) float32, faces (n, 3) int32) of a PLY exactly as write_ply writes it."""
    buf = open(path, "rb").read()
    end = buf.find(b"end_header\n")
    if not buf.startswith(b"ply\nformat binary_little_endian 1.0\n") or end < 0:
        raise ValueError("not a binary little-endian PLY")
    nv = nf = None
    for line in buf[:end].split(b"\n"):
        f = line.split()
        if f[:2] == [b"element", b"vertex"]:
            nv = int(f[2])
        elif f[:2] == [b"element", b"face"]:
            nf = int(f[2])
    if nv is None or nf is None:
        raise ValueError("PLY header without vertex / face elements")
    off = end + len(b"end_header\n")
    if len(buf) != off + 12 * nv + 13 * nf:
        raise ValueError("PLY body size does not match its header")
    verts = np.frombuffer(buf, "<f4", 3 * nv, off).reshape(nv, 3).copy()
    rec = np.frombuffer(buf, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, off + 12 * nv)
    if nf and not (rec["n"] == 3).all():
        raise ValueError("PLY face that is not a triangle")
    return verts, rec["v"].astype(np.int32)


def read_ply_attr(path):
    """(vertices (m, 3) float32, faces (n, 3) int32, normals (m, 3) float32 or None, colours (m, 4)
    uint8 RGBA or None) of a PLY as write_ply writes it, by the header's property list."""
    buf = open(path, "rb").read()
    end = buf.find(b"end_header\n")
    if not buf.startswith(b"ply\nformat binary_little_endian 1.0\n") or end < 0:
        raise ValueError("not a binary little-endian PLY")
    types = {b"float": "<f4", b"uchar": "u1", b"int": "<i4"}
    nv = nf = None
    element, props = None, []
    for line in buf[:end].split(b"\n"):
        f = line.split()
        if f[:1] == [b"element"]:
            element = f[1]
            if element == b"vertex":
                nv = int(f[2])
            elif element == b"face":
                nf = int(f[2])
        elif f[:1] == [b"property"] and element == b"vertex":
            if f[1] not in types:
                raise ValueError("PLY vertex property of an unknown type")
            props.append((f[2].decode(), types[f[1]]))
    if nv is None or nf is None:
        raise ValueError("PLY header without vertex / face elements")
    vdt = np.dtype(props)
    names = vdt.names or ()
    if names[:3] != ("x", "y", "z"):
        raise ValueError("PLY vertices without x y z")
    off = end + len(b"end_header\n")
    if len(buf) != off + vdt.itemsize * nv + 13 * nf:
        raise ValueError("PLY body size does not match its header")
    v = np.frombuffer(buf, vdt, nv, off)
    cols = lambda ns, dt: np.stack([v[k] for k in ns], -1).astype(dt) if nv else np.zeros((0, len(ns)), dt)
    verts = cols(("x", "y", "z"), np.float32)
    normals = cols(("nx", "ny", "nz"), np.float32) if all(k in names for k in ("nx", "ny", "nz")) else None
    colours = cols(("red", "green", "blue", "alpha"), np.uint8) if all(k in names for k in ("red", "green", "blue", "alpha")) else None
    rec = np.frombuffer(buf, np.dtype([("n", "u1"), ("v", "<i4", 3)]), nf, off + vdt.itemsize * nv)
    if nf and not (rec["n"] == 3).all():
        raise ValueError("PLY face that is not a triangle")
    return verts, rec["v"].astype(np.int32), normals, colours
