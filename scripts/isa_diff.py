"""Which device functions' machine code differs between two builds of mc_api.hip (gfx950 device assembly from
`hipcc -S --offload-device-only`).  The S1 class kernels have shown build-dependent results (DESIGN.md
§4, round-4 investigation), so a source change is validated against the GPU runs of the build whose
code it reproduces: an unchanged function list means the tested machine code ships.

    python scripts/isa_diff.py <git-rev> [name-substring] [-DNAME[=VALUE] ...]

compares <git-rev>'s source with the working tree; the -D arguments go to both compiles (the diagnostics
and stamps builds).  Only symbols the assembly types as functions are compared, every one of them unless a
substring of the mangled name is given (`k_bp`: the S1 kernels).  Local labels carry the function's index in
the code object (`.LBB<n>_<m>`, `.LJTI<n>_<m>`), and so do the compiler's comments behind a line (`; in Loop:
Header=BB<n>_<m>`); the index and the comments are dropped before comparing, so a function that only changed
its place is reported identical.  Exit status 1 when any function differs or exists on one
side only.
"""
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--offload-device-only"]
LOCAL_LABEL = re.compile(r"\.(LBB|LJTI)\d+_")


def functions(s):
    """mangled name -> instruction lines, from the text of a device assembly file"""
    is_func = set(re.findall(r"^\s*\.type\s+(\S+),@function", s, re.M))
    funcs = {}
    for m in re.finditer(r"^([A-Za-z_$][\w.$]*):", s, re.M):
        if m.group(1) not in is_func:
            continue
        end = s.find(".Lfunc_end", m.end())
        funcs[m.group(1)] = [LOCAL_LABEL.sub(r".\1_", l.split(";")[0].rstrip()) for l in s[m.end():end].splitlines()
                             if l.strip() and not l.strip().startswith((".loc", ";", ".Ltmp", ".cfi"))]
    return funcs


def device_asm(src_dir, out, defines):
    subprocess.check_call(["/opt/rocm/bin/hipcc", *FLAGS, *defines, os.path.join(src_dir, "mc_api.hip"), "-o", out],
                          stderr=subprocess.DEVNULL)
    return functions(open(out).read())


def report(a, b, sub):
    names = sorted(k for k in set(a) | set(b) if sub in k)
    diff = [k for k in names if a.get(k) != b.get(k)]
    for k in diff:
        print("differs:", k, len(a.get(k, [])), len(b.get(k, [])))
    print(f"{len(names) - len(diff)} of {len(names)} functions matching '{sub}' identical "
          f"({sum(sub in k for k in a)} before, {sum(sub in k for k in b)} after)")
    return 1 if diff else 0


def main():
    defines = [a for a in sys.argv[1:] if a.startswith("-D")]
    args = [a for a in sys.argv[1:] if not a.startswith("-D")]
    rev = args[0]
    sub = args[1] if len(args) > 1 else ""
    with tempfile.TemporaryDirectory() as tmp:
        wt = os.path.join(tmp, "wt")
        subprocess.check_call(["git", "-C", REPO, "worktree", "add", "-f", "-q", wt, rev])
        try:
            a = device_asm(os.path.join(wt, "maskclustering_amd", "csrc"), os.path.join(tmp, "a.s"), defines)
        finally:
            subprocess.call(["git", "-C", REPO, "worktree", "remove", "--force", wt])
        b = device_asm(os.path.join(REPO, "maskclustering_amd", "csrc"), os.path.join(tmp, "b.s"), defines)
    return report(a, b, sub)


if __name__ == "__main__":
    sys.exit(main())
