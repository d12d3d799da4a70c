"""S1 ball query cell arithmetic (maskclustering_amd/csrc/mc_bp_qcell.hpp): the cell range of a mask's float32
box on the 2r scene grid and the numbering of its cells are plain host/device functions; k_bp_query_lds stages
a slot's cropped scene points by them.  scripts/bp_qcell_check.cpp checks, as a stand-alone program under the
address and undefined-behaviour sanitizers, that the range holds the cell of every point strictly inside the box
(random floats, floats on and next to cell borders and box corners, the kCellBias clamps) and that the numbering
is a bijection onto [0, cells) whose x-neighbours are consecutive (the GPU tests in test_gpu_s1_query.py run the
same functions inside the kernel)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_box_cells_hold_inside_points_and_numbering_is_a_bijection(tmp_path):
    exe = tmp_path / "bp_qcell_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_qcell_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
