"""The whole indexed mesh's reference (tests/mesh_indexed_whole_ref.py) on the CPU: the hand-made two-tier
scene covers what the slot-keyed kernels can get wrong -- these are conditions on the INPUT of the GPU tests
(tests/test_gpu_mesh_indexed_whole.py) -- and the streaming PLY writer under sanitizers, chunk by chunk, against
the one-call writer."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import mesh_indexed_ref as X
import mesh_indexed_whole_ref as XW
import mesh_ref as M
import mesh_whole_ref as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    return XW.two_tier_indexed()


@pytest.fixture(scope="module")
def owners(case):
    return XW.ownership(case["hash"], case["vba"], case["state"], case["flags"], case["store"], M.RANDOM["n_buckets"])


def test_composition(case):
    """The composition is an indexed form of the whole reading: it dereferences to the whole soup, every vertex is
    referenced, and it is a real scene (counts given for orientation in the issue: 43 320 triangles, 34 949 vertices)."""
    v, i, n = case["vertices"], case["indices"], case["vnormals"]
    assert len(i) == len(case["tris"]) > 10000 and len(v) == len(n) > 10000
    assert v[i].tobytes() == np.ascontiguousarray(case["tris"]).tobytes()
    assert n[i].tobytes() == np.ascontiguousarray(case["normals"]).tobytes()
    assert np.array_equal(np.unique(i), np.arange(len(v))), "an unreferenced vertex"
    assert i.dtype == np.uint32 and v.dtype == n.dtype == np.float32


def test_edges_are_not_welded(case):
    assert len(case["vertices"]) > len(M.weld(case["tris"])[0]), "no two distinct edges with bit-equal positions"


def test_owner_offsets_and_excess(case):
    st = case["stats"]
    assert st["owner_dirs"] == set(itertools.product((0, 1), repeat=3)) - {(1, 1, 1)}, st["owner_dirs"]
    assert st["excess_owners"] > 0, "no owner entry in the excess list"


def test_every_resolving_class_emits_and_owns_foreign_edges(case, owners):
    """Each of the four resolving classes occurs as an emitting entry, and each owns an edge of ANOTHER entry's
    triangle: the cross-entry, slot-keyed lookup runs in every tier.  Lost entries emit and own nothing."""
    cls = case["cls"]
    ent, owner = owners
    assert len(ent) == len(case["indices"])
    assert (owner >= 0).all()
    emitting = np.bincount(cls[np.unique(ent)], minlength=5)
    foreign = owner[owner != ent[:, None]]
    own_foreign = np.bincount(cls[foreign], minlength=5)
    for k in range(4):
        assert emitting[k] > 0, f"no emitting entry of class {WR.CLASSES[k]}"
        assert own_foreign[k] > 0, f"class {WR.CLASSES[k]} owns no edge of another entry's triangle"
    lost = np.nonzero(cls == 4)[0]
    assert len(lost) > 0
    assert emitting[4] == 0 and not np.isin(owner, lost).any(), "a lost entry emits or owns"
    assert (cls[owner] >= 0).all(), "an unallocated entry owns"
    # the vertex numbering is the owner's order: ascending owner entry along the vertex table
    first_owner = np.full(len(case["vertices"]), -1, np.int64)
    first_owner[case["indices"].reshape(-1)] = owner.reshape(-1)
    assert (np.diff(first_owner) >= 0).all()


def test_resident_form_of_the_case_differs(case):
    """The resident indexed mesh of the same tables (unresolved) is another mesh: the GPU test that alternates
    the two forms on one context compares different things."""
    rv, ri, _, _ = X.indexed(case["hash"], case["vba"], M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    assert 0 < len(ri) < len(case["indices"]) and 0 < len(rv) < len(case["vertices"])


def test_other_seed_has_other_slots():
    """The scratch-life test's second scene: another seed resolves other entries, so its slots differ."""
    a, b = XW.two_tier_indexed(), XW.two_tier_indexed(1)
    ra = WR.classify(a["hash"], a["state"], a["flags"]) >= 0
    rb = WR.classify(b["hash"], b["state"], b["flags"]) >= 0
    assert ra.sum() > 0 and rb.sum() > 0 and not np.array_equal(ra, rb)
    assert a["indices"].tobytes() != b["indices"].tobytes()


def test_no_stored_data_is_resident():
    h, vba, _, _ = M.random_case()
    z = np.zeros(len(h), np.uint8)
    store = np.zeros(len(h) * 512, vba.dtype)
    v, i, n = XW.indexed_whole(h, vba, z, z, store, M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    rv, ri, rn, _ = X.indexed(h, vba, M.VOXEL_SIZE, M.RANDOM["n_buckets"])
    assert v.tobytes() == rv.tobytes() and i.tobytes() == ri.tobytes() and n.tobytes() == rn.tobytes() and len(i) > 0


def test_ply_stream_under_asan_ubsan(tmp_path):
    """tf_mesh_ply.cpp built for the CPU with -fsanitize=address,undefined and driven by tests/mesh_ply_stream_main.cpp:
    chunks of 1 record, ragged last chunks and one chunk holding everything give the one-call writer's file byte for
    byte, for every column combination and for nv = 0; an out-of-range index in a late chunk, miscounted records and
    bad arguments are refused and leave no file -- with no sanitizer report."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mesh_ply_stream_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "mesh_ply_stream_main.cpp"),
                        os.path.join(ROOT, "topfusion_amd", "csrc", "tf_mesh_ply.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = tmp_path / "files"
    out.mkdir()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    assert not (out / "bad.ply").exists()
