"""Scene point cloud fusion of a TASMap-shaped capture, in one process:
  (device)  mc_cloud_fuse_frames with the frames resident on the device, and the same with the frames
            on the host (the upload of depth and colour included);
  (host)    the numpy restatement (tests/scene_cloud_restatement.py), one process, once.
The parent commit has no device route and Open3D is not installed, so the restatement is the only
baseline, and its result is the witness: the device result must equal it bit for bit.
Input: --frames synthetic frames of --size x --size (default 60 of 1024 x 1024), --buffer frames a
buffer (30), voxel 0.005.  Device time: wall clock around the call (it waits for its result), one
warm-up, then --repeats runs (median, min, max); the per-kernel timers of one further run; cloud_info.
Prints one JSON line.
GPU run: python scripts/scene_cloud_ab.py [--frames 60] [--size 1024] [--buffer 30] [--repeats 5] [--no-host]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import scene_cloud_restatement as R  # noqa: E402
from maskclustering_amd import _native  # noqa: E402

TIMERS = ("cloud_input", "cloud_bounds", "cloud_hash", "cloud_order", "cloud_lists", "cloud_fold_small",
          "cloud_fold_lds", "cloud_fold_global")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=60)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--buffer", type=int, default=30)
    ap.add_argument("--voxel", type=float, default=0.005)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the restatement (no bit-equality check)")
    a = ap.parse_args()
    S = a.size
    depth, rgb, K, T = R.synthetic_frames(a.frames, S, S, seed=0, focal=0.8 * S)
    T = np.ascontiguousarray(T)
    ctx = _native.Context(0)
    prm = _native.CloudParams(a.voxel, 20.0, a.buffer)
    dev = [torch.from_numpy(x).to("cuda:0") for x in (depth, rgb, K, T)]
    torch.cuda.synchronize()

    def timed(args):
        ms = []
        ctx.cloud_fuse(*args, prm)  # warm-up
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ctx.cloud_fuse(*args, prm)
            ms.append((time.perf_counter() - t0) * 1e3)
        return dict(median=round(float(np.median(ms)), 2), min=round(min(ms), 2), max=round(max(ms), 2), repeats=a.repeats)

    device_ms = timed(dev)
    host_ms = timed((depth, rgb, K, T))
    ctx.set_timing(True)
    ctx.reset_kernel_times()
    info = ctx.cloud_fuse(*dev, prm)
    ctx.synchronize()
    kernels = {k: round(ctx.kernel_time(k)[0], 3) for k in TIMERS}
    ctx.set_timing(False)
    got_p, got_c = ctx.cloud_get()
    out = {"what": "scene point cloud fusion: device route vs the numpy restatement (one process)",
           "device": torch.cuda.get_device_name(0), "frames": [a.frames, S, S], "buffer_frames": a.buffer,
           "voxel_size": a.voxel, "device_resident_ms": device_ms, "from_host_ms": host_ms, "device_kernels_ms": kernels,
           "cloud_info": info}
    if not a.no_host:
        t0 = time.perf_counter()
        rinfo = {}
        want_p, want_c = R.fuse_frames(depth, rgb, K, T, a.voxel, a.buffer, info=rinfo)
        out["restatement_s"] = round(time.perf_counter() - t0, 2)
        out["bit_equal"] = bool(got_p.shape == want_p.shape and got_p.tobytes() == want_p.tobytes() and
                                got_c.tobytes() == want_c.tobytes())
        out["restatement_over_device"] = round(out["restatement_s"] * 1e3 / device_ms["median"], 1)
        pops = np.concatenate(rinfo["populations"])
        out["voxels_by_class"] = {"thread": int((pops <= 16).sum()), "lds": int(((pops > 16) & (pops <= 4096)).sum()),
                                  "global": int((pops > 4096).sum())}
        print(json.dumps(out), flush=True)
        assert out["bit_equal"], "the device result differs from the restatement"
    else:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
