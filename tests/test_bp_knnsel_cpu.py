"""S1 denoise k-NN candidate selection (maskclustering_amd/csrc/mc_bp_knnsel.hpp).  scripts/bp_knnsel_check.cpp,
a stand-alone program built with -ffp-contract=off, checks on the CPU: the distance class is monotone in d2
(10^6 draws per eps, each against its neighbours up and down, the class boundaries, the clamp just below
eps2); the packed histogram's threshold against a cumulative scan (totals below, at and above k, one class,
counts of 64); the sorting network on every 0-1 input of its 24 lines (bit-sliced) and its first 20 outputs
on values with ties; and the whole selection (class -> histogram -> selected set -> network -> leftover
inserts) against std::sort and std::accumulate, bit for bit, on lists with ties, kept flags and selected sets
larger than the network.  A second build runs under the address and undefined-behaviour sanitizers.  The GPU
tests in test_gpu_s1_knnsel.py run the same functions inside the class kernels."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",),
                                   ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_knn_selection_equals_sort_bit_for_bit(tmp_path, flags):
    exe = tmp_path / "bp_knnsel_check"
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_knnsel_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "net=24" in r.stdout and "bad=0" in r.stdout, r.stdout + r.stderr
