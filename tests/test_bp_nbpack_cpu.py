"""S1 denoise list packing (maskclustering_amd/csrc/mc_bp_nbpack.hpp): the register packing of eps-list
entries into 16-byte words, the store rules (a full word at every multiple of 8, one partial last word with
zero padding, nothing past the cap) and the consumers' slot extraction are plain host/device functions;
scripts/bp_nbpack_check.cpp builds lists of 0 .. 66 entries with them as the kernel's builder does and reads
them back as the consumers do, as a stand-alone program under the address and undefined-behaviour sanitizers
(the GPU tests in test_gpu_s1.py and test_gpu_s1_lists.py run the same functions inside k_bp_denoise_lds)."""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_list_packing_counts_flushes_cap_and_round_trip(tmp_path):
    exe = tmp_path / "bp_nbpack_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "bp_nbpack_check.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
