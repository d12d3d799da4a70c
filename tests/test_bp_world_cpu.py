"""S1 voxels: a pixel's world point (maskclustering_amd/csrc/mc_bp_world.hpp).  The voxel kernels choose per
slot between the general form (four pose rows and a homogeneous divide) and the affine form (three rows, no
divide) by bp_pose_affine; the choice must not change one bit of any point.  scripts/bp_world_check.cpp, a
stand-alone program built with -ffp-contract=off, compares the two forms' 64-bit patterns on 1.2 * 10^6
draws of rigid poses, dataset intrinsics, pixels in [0, 65535]^2 and float depths in (0, trunc) (signed zeros
in row 3, negative and huge translations, the smallest normal and denormal depths, a NaN in rows 0-2), checks
what the predicate rejects (row-3 entries one ulp off, T[15] = 2, non-finite or zero fx / fy, non-finite
cx / cy), and checks that the slot minimum taken without the translation and shifted once equals the minimum
of the points.  A second build runs under the address and undefined-behaviour sanitizers.  The GPU tests in
test_gpu_s1_world.py run the same functions inside the three voxel kernels."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags, draws", [(("-O2",), 1200000),
                                          (("-O1", "-g", "-fsanitize=address,undefined",
                                            "-fno-sanitize-recover=undefined"), 200000)],
                         ids=["plain", "sanitized"])
def test_affine_world_point_equals_general_bit_for_bit(tmp_path, flags, draws):
    exe = tmp_path / "bp_world_check"
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_world_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(draws)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"draws={draws}" in r.stdout and "bad=0" in r.stdout, r.stdout + r.stderr
