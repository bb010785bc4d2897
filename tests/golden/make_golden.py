"""Regenerates the reference-pinned golden vectors in tests/golden/ (run in the build
container, where /root/reference exists; the GPU box only reads the committed files).

  1. `make -C oracle ref` compiles oracle/ref_pin/ref_pin.cpp against the reference's own,
     self-contained headers (tfusion/include/Math.hpp, Vector.hpp, Matrix.hpp,
     MathUtils.hpp, tfusion/cuda/VoxelTypes.hpp, tfusion/cuda/PixelUtils.hpp) into
     oracle/_ref/ref_pin -- no stand-in
     headers, nothing from the reference is copied into the repo.
  2. oracle/_ref/ref_pin writes ref_pin_{inv,m4v,round,voxel,bilinear,colour}.bin here (raw little-endian
     f32 records; layouts in tests/test_oracle.py).
  3. The same make target compiles oracle/ref_pin/ref_pin_stages.cpp against the reference's shared
     per-element headers (declaration-only stand-ins for OpenCV and CUDA) into
     oracle/_ref/ref_pin_stages.  For every scene of tests/pin_scenes.py it reads the scene and the
     cases' inputs from a temporary pin file and writes stage_pin_<scene>_<case>.bin; the coverage
     conditions (pin_scenes.check_coverage) are asserted before a file is put here (layouts in
     tests/test_oracle_stage_pin.py).

  4. The same make target compiles oracle/ref_pin/ref_pin_front.cpp: the reference's imgproc.cu and proj_icp.cu
     themselves, for the host, over the executing CUDA stand-ins of oracle/ref_pin/cuda_exec.  For every case of
     tests/front_pin_cases.py it writes front_pin_<case>_p<k>.bin (layouts there); the coverage conditions are
     asserted before a file is put here, and stale parts of a case are removed.

    python tests/golden/make_golden.py
"""
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def run_stage_pin(exe, out_dir):
    """Runs the stage pin program over every scene into out_dir and checks the coverage conditions."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import pin_scenes as P
    for scene in P.SCENES:
        src = os.path.join(out_dir, scene + ".in")
        P.write_pin(src, P.pin_inputs(scene))
        subprocess.run([exe, src, out_dir, scene], check=True, stdout=subprocess.DEVNULL)
        os.remove(src)
        for case in P.CASES:
            path = os.path.join(out_dir, os.path.basename(P.golden_path(scene, case)))
            if not os.path.exists(path):            # a pin program built without SceneReconstructionEngine.hpp
                print(f"skipped: {scene} {case} (the committed golden stays as it is)")
                continue
            P.check_coverage(case, P.read_pin(path))
            assert os.path.getsize(path) <= P.MAX_GOLDEN_BYTES, (path, os.path.getsize(path))


def run_front_pin(exe, out_dir):
    """Runs the front pin program over every case into out_dir and checks the coverage conditions."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import front_pin_cases as F
    import pin_scenes as P
    from oracle import oracle as O
    jobs = [(F.front_case(W, H), lambda W=W, H=H: F.front_inputs(W, H)) for W, H in F.FRONT_SIZES]
    jobs += [(F.icp_case(W, H), lambda W=W, H=H: F.icp_inputs(O, W, H)) for W, H in F.ICP_SIZES]
    for case, inputs in jobs:
        src = os.path.join(out_dir, case + ".in")
        P.write_pin(src, inputs())
        subprocess.run([exe, src, out_dir, case], check=True, stdout=subprocess.DEVNULL)
        os.remove(src)
        for path in F.golden_parts(case, out_dir):
            assert os.path.getsize(path) <= P.MAX_GOLDEN_BYTES, (path, os.path.getsize(path))
    for W, H in F.FRONT_SIZES:
        F.check_front_coverage(W, H)
    for W, H in F.ICP_SIZES:
        F.check_icp_coverage(F.golden(F.icp_case(W, H), out_dir), W, H)


def main():
    if not os.path.isdir("/root/reference/tfusion/include"):
        sys.exit("reference tree absent: the committed goldens stay as they are")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref"], check=True)
    subprocess.run([os.path.join(ROOT, "oracle", "_ref", "ref_pin"), HERE], check=True)
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_pin_stages")
    if not os.path.exists(exe):
        sys.exit("oracle/_ref/ref_pin_stages was not built: the stage_pin goldens stay as they are")
    with tempfile.TemporaryDirectory() as tmp:
        run_stage_pin(exe, tmp)
        front = os.path.join(ROOT, "oracle", "_ref", "ref_pin_front")
        if os.path.exists(front):
            run_front_pin(front, tmp)
            for name in os.listdir(HERE):
                if name.startswith("front_pin_") and name.endswith(".bin"):
                    os.remove(os.path.join(HERE, name))
        else:
            print("oracle/_ref/ref_pin_front was not built: the front_pin goldens stay as they are")
        for name in sorted(os.listdir(tmp)):
            shutil.copyfile(os.path.join(tmp, name), os.path.join(HERE, name))
            print("wrote", name)


if __name__ == "__main__":
    main()
