"""Graph and clustering host decisions (maskclustering_amd/csrc/mc_graph_plan.hpp): the frame starts,
the shard row cut, the S3 work lists, the S4 histogram replica count, the S6 mode and the components
route are pure host functions; scripts/graph_plan_check.cpp asserts worked cases of each (the row cut's
from the restatement in oracle_shard_ctx.py), the row cut's structure on 3000 random offset tables and
the work lists against std::stable_sort on 1500 random size tables, as a stand-alone program under the
address and undefined-behaviour sanitizers (the GPU tests run the same functions inside
mc_scene_set_masks, mc_shard_set and mc_cluster_run)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_graph_plan_worked_cases_row_cut_structure_and_work_lists(tmp_path):
    exe = tmp_path / "graph_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "graph_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
