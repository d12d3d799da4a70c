"""Post-processing host decisions (maskclustering_amd/csrc/mc_pp_plan.hpp): the items of the split
DBSCAN's big nodes, the objects filter_point keeps, the greedy merge over the list of non-zero decisions
and the final-object tables are pure host functions; scripts/pp_plan_check.cpp asserts worked cases of
each and compares the greedy merge, on 2000 shuffled random decision lists, with a dense restatement of
post_process.py:14-29, as a stand-alone program under the address and undefined-behaviour sanitizers
(the GPU tests in test_gpu_pp.py and test_gpu_pp_device.py run the same functions inside mc_pp_run*)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pp_plan_worked_cases_and_greedy_merge_against_dense_loop(tmp_path):
    exe = tmp_path / "pp_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "pp_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
