"""Label painter host decisions and bit arithmetic (maskclustering_amd/csrc/mc_paint_plan.hpp): the
refusals with their messages, the rounds of frames against a budget, the float32 selection and the
stable order at their edges, and the kernels' three bit tricks (mask bytes to bits, the bit-sliced
fold, the 8 x 8 transpose) are pure functions; scripts/paint_plan_check.cpp asserts them as a
stand-alone program under the address and undefined-behaviour sanitizers
(tests/test_gpu_label_paint.py runs the same functions inside mc_labels_paint)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_paint_plan_refusals_rounds_order_and_bit_tricks(tmp_path):
    exe = tmp_path / "paint_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "paint_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
