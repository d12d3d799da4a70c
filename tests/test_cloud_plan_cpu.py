"""Scene point cloud host decisions (maskclustering_amd/csrc/mc_cloud_plan.hpp): the flush schedule of
(F, buffer_frames), the table size, a stage's bytes against the budget and the refusals with their
messages, the 2^21 extent rule, the voxel index and the comparator schedule of the per-voxel sort are
pure functions; scripts/cloud_plan_check.cpp asserts them as a stand-alone program under the address
and undefined-behaviour sanitizers (tests/test_gpu_scene_cloud.py runs the same functions inside
mc_cloud_fuse_frames and mc_cloud_voxel_down)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cloud_plan_schedule_sizes_refusals_and_sort_network(tmp_path):
    exe = tmp_path / "cloud_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I",
                           os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "cloud_plan_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
