"""Helpers of the evaluation-state tests (tests/test_gpu_ap_state.py, tests/ap_state_worker.py): the
state buffer of include/mcgraph.h (mc_ev_state_*) restated in numpy, the buffer expected from an
APRestatement, and a launcher for the worker processes."""
import os
import socket
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STATE_WORD = (1 << 32) | 0x5645434D                      # version 1, "MCEV"
SECTIONS = ("class_ids", "overlaps", "run_off", "hard_fn", "flags", "key", "n_true", "n_false")


def key_of(score):
    """The sortable key of a score (mc_ap_kernels.inl, ev_key): -0.0 as 0.0."""
    b = int((np.float64(score) + 0.0).view(np.uint64))
    return (~b) & (2 ** 64 - 1) if b >> 63 else b | (1 << 63)


def layout(C, O, R):
    """Byte offset and dtype of every section, and the buffer's size."""
    up = lambda n: (n + 7) & ~7                          # noqa: E731
    NC = C * O
    off, at = {}, 48
    for name, dt, n in (("class_ids", np.int32, C), ("overlaps", np.float64, O), ("run_off", np.int64, NC + 1),
                        ("hard_fn", np.int64, NC), ("flags", np.uint32, NC), ("key", np.uint64, R), ("n_true", np.uint32, R),
                        ("n_false", np.uint32, R)):
        off[name] = (at, np.dtype(dt), n)
        at += up(n * np.dtype(dt).itemsize)
    return off, at


def parse_state(buf):
    """The buffer's header words and sections (copies)."""
    buf = np.asarray(buf, np.uint8)
    word, C, O, mrs, nc, R = (int(x) for x in buf[:48].view(np.int64))
    off, size = layout(C, O, R)
    assert size == len(buf), (size, len(buf))
    st = dict(word=word, C=C, O=O, min_region_size=mrs, no_class=nc, R=R)
    for name, (at, dt, n) in off.items():
        st[name] = buf[at:at + n * dt.itemsize].view(dt).copy()
    return st


def build_state(st):
    """The buffer of parse_state's dict (R is taken from the header word given, not from the sections)."""
    C, O, R = st["C"], st["O"], len(st["key"])
    off, size = layout(C, O, R)
    buf = np.zeros(size, np.uint8)
    buf[:48].view(np.int64)[:] = (st["word"], C, O, st["min_region_size"], st["no_class"], st["R"])
    for name, (at, dt, n) in off.items():
        buf[at:at + n * dt.itemsize].view(dt)[:] = np.asarray(st[name], dt)
    return buf


def expected_state(rs):
    """The state buffer of an APRestatement's accumulation."""
    C, O = rs.C, rs.O
    run_off, key, nt, nf = [0], [], [], []
    for c in range(C):
        for o in range(O):
            runs = {}
            for s in rs.scans:
                for score, true in s.get((c, o), []):
                    r = runs.setdefault(key_of(score), [0, 0])
                    r[0 if true else 1] += 1
            for k in sorted(runs):
                key.append(k), nt.append(runs[k][0]), nf.append(runs[k][1])
            run_off.append(len(key))
    return build_state(dict(word=STATE_WORD, C=C, O=O, min_region_size=rs.min_region_size, no_class=int(rs.no_class),
                            R=len(key), class_ids=rs.class_ids, overlaps=rs.overlaps, run_off=run_off,
                            hard_fn=rs.hard_fn.ravel(), flags=rs.flags.ravel(), key=np.array(key, np.uint64),
                            n_true=nt, n_false=nf))


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def run_workers(mode, world, tmpdir, backend="gloo", timeout=120):
    """tests/ap_state_worker.py once per rank (at most 4), each under its own time limit; one failure or
    timeout ends the others.  Returns the ranks' output files."""
    assert 1 <= world <= 4
    port = free_port()
    tag = mode.replace(":", "_")
    outs = [os.path.join(str(tmpdir), f"{tag}_{world}_{r}.npz") for r in range(world)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="2")
    logs = [open(os.path.join(str(tmpdir), f"{tag}_{world}_{r}.log"), "w+") for r in range(world)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "ap_state_worker.py"), mode, backend, str(r), str(world),
                               str(port), outs[r]], env=env, stdout=logs[r], stderr=subprocess.STDOUT)
             for r in range(world)]
    t0 = time.monotonic()
    failed = None
    try:
        left = set(range(world))
        while left and failed is None:
            for r in sorted(left):
                try:
                    rc = procs[r].wait(timeout=0.05)
                except subprocess.TimeoutExpired:
                    if time.monotonic() - t0 > timeout:
                        failed = (r, "its time limit")
                        break
                    continue
                left.discard(r)
                if rc != 0:
                    failed = (r, rc)
                    break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    text = []
    for f in logs:
        f.seek(0)
        text.append(f.read())
        f.close()
    assert failed is None, f"rank {failed[0]} exited with {failed[1]}:\n{text[failed[0]][-3000:]}"
    return outs
