"""S1 denoise ring search (maskclustering_amd/csrc/mc_bp_ring.hpp).  scripts/bp_ring_check.cpp, a stand-alone
program built with -ffp-contract=off, checks on the CPU: the enumeration of the 27 cells of the inner ring and
the 98 of the shell visits each cell once; the mask returns its marked cells once each; the gap of a cell is
never above the computed distance to a point in it; and mark and walk, run as k_bp_knn_ring runs them over a
hashed grid (with the class kernel's 2 n buckets, with 7 and with 1, so that the cells of a ring share buckets),
leave the same 20 smallest squared distances as a brute-force scan of the ring's cells, bit for bit, on random
and lattice clouds, surface patches, edge strips and clouds of 20 to 40 points; no cell that holds a point
below the ring's final k-th distance is left unmarked.  A second build runs under the address and
undefined-behaviour sanitizers.  The GPU tests in test_gpu_s1_ring.py run the same functions inside the kernel."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O2",),
                                   ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined")],
                         ids=["plain", "sanitized"])
def test_ring_search_equals_brute_force_bit_for_bit(tmp_path, flags):
    exe = tmp_path / "bp_ring_check"
    subprocess.check_call(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-ffp-contract=off",
                           "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_ring_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "r1=" in r.stdout and "bad=0" in r.stdout, r.stdout + r.stderr
