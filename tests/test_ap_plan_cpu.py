"""AP evaluation host decisions (maskclustering_amd/csrc/mc_ap_plan.hpp): the table rules of
mc_ev_add_matches, the class slots and the word block of a scan, the 2^31 limit, the unpacking of the
compact tables and the header and section checks of the state buffer are pure host functions;
scripts/ap_plan_check.cpp asserts a worked scan word for word, every rejection with its message and the
precedence among them, 2000 random tables against a restatement, and a state buffer built there with
every rejection the host decides, as a stand-alone program under the address and undefined-behaviour
sanitizers (the GPU tests in test_gpu_ap.py and test_gpu_ap_state.py run the same functions inside
mc_ev_add_* and mc_ev_state_merge)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ap_plan_worked_cases_rejections_and_random_tables_against_a_restatement(tmp_path):
    exe = tmp_path / "ap_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "ap_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
