"""The host-only code of the free views under AddressSanitizer and UBSan, on the CPU: tests/view_host_main.cpp (a
stand-alone program) drives the registry of a context's live views (TfCtxViews, tf_ctx_mem.h) and the PPM writer
(tfusion::io::writePPM).  Plus what the C-ABI's header and its Python binding must agree on."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_view_registry_and_ppm_writer_under_asan_ubsan(tmp_path):
    """add / remove / live / count of TfCtxViews, the drop of the views still alive at destruction (newest first,
    each once), a second remove and a foreign pointer refused; writePPM of a pitched and of a packed RGBA image
    against the bytes expected, read back by readPPM, and its four refusals."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "view_host_main")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "view_host_main.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = tmp_path / "out"
    out.mkdir()
    r = subprocess.run([exe, str(out)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 5 views, 56 ppm bytes") and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr


def test_view_functions_are_declared_and_bound():
    """Every tf_view_* function of include/tfusion_hip.h has a ctypes signature, and the enum values agree."""
    from topfusion_amd import _lib
    names = [n for n in _lib.header_functions() if n.startswith("tf_view_")]
    assert sorted(names) == sorted(["tf_view_create", "tf_view_destroy", "tf_view_get_params", "tf_view_find_visible",
                                    "tf_view_expected_depths", "tf_view_raycast", "tf_view_shade", "tf_view_icp_maps",
                                    "tf_view_render", "tf_view_download", "tf_view_stats"])
    src = open(_lib.HEADER_PATH).read()
    for k, name in enumerate(("TF_VIEW_VISIBLE_IDS", "TF_VIEW_RANGE", "TF_VIEW_RAYCAST", "TF_VIEW_IMAGE")):
        assert f"{name} = {k}" in src and getattr(_lib, name) == k
    L = _lib.load()
    for n in names:
        assert getattr(L, n).argtypes is not None, n
