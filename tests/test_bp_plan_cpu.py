"""S1 batch planning (maskclustering_amd/csrc/mc_bp_plan.hpp): the byte budget, the pixel budget, the
frames per batch with their equal dealing, the mask-pixel capacity and the shrink after an overflow are
pure host functions; scripts/bp_plan_check.cpp asserts worked cases of each and that the grow-and-redo
loop built from them terminates, as a stand-alone program under the address and undefined-behaviour
sanitizers (the GPU tests in test_gpu_s1.py run the same functions inside mc_backproject)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_worked_cases_and_redo_termination(tmp_path):
    exe = tmp_path / "bp_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
