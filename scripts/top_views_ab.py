"""Projected boxes of one scene's top views, three routes, in one process:
  (resident) mc_proj_top_views(top_k) on the post-processed scene, camera arrays and outputs on the
             device: selection of the top views, projection and boxes with nothing crossing to the host;
  (host in)  mc_proj_boxes given the same requests and the mc_pp_export arrays as host arrays
             (uploads, the call's own wait and the read-back included);
  (numpy)    the numpy restatement (tests/top_views_restatement.py) looping over the same requests, as
             the reference's get_bbox_by_projection does per (object, frame), one process.
The parent commit has no device route, so the numpy route is the baseline.  The scene is a synthetic
C2-shaped one (synthetic_frames); the requests are the first top_k masks of every final object by
coverage.  Resident time: events on the context's stream, one warm-up, then --repeats runs (median,
min, max), and the per-kernel timers of one further run.  Host-in and numpy: wall clock (host-in:
median of --repeats; numpy: one pass).  The three routes' boxes, status and in-bounds counts are
compared on every request.  Achieved GB/s is against the algorithmic bytes: per requested object
|points| * (4 + 24) B, read once for all of its frames.  Prints one JSON line.
GPU run: python scripts/top_views_ab.py [--shape c2] [--top-k 9] [--repeats 9]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import bench  # noqa: E402
import top_views_restatement as R  # noqa: E402
from maskclustering_amd._native import PPParams  # noqa: E402
from maskclustering_amd.synthetic_frames import make_frames_shape  # noqa: E402

TIMERS = ("proj_select", "proj_boxes")


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--top-k", type=int, default=9)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    from maskclustering_amd.sweep import SceneSweep
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
        sw = SceneSweep(0, bench.shape_thresholds(a.shape)[1], stream=stream.cuda_stream)
        ctx = sw.ctx
        fr = make_frames_shape(a.shape, seed=0, device="cuda:0")   # rendered on the device, returned as numpy
        sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                     t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64),
                     post_process=PPParams(0.1, 4, 0.5, 0.8))
        F, H, W = (int(v) for v in fr.seg.shape)
        k = np.ascontiguousarray(fr.intrinsics, np.float64).reshape(-1, 4)
        w2c = np.linalg.inv(np.asarray(fr.poses, np.float64).reshape(-1, 4, 4))
        k_d, w2c_d = t(k, torch.float64), t(w2c, torch.float64)

        def resident():
            return ctx.proj_top_views(k_d, w2c_d, W, H, top_k=a.top_k, device=True)

        out = resident()                                   # warm-up: buffers sized, the export arrays built
        stream.synchronize()
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            resident()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ctx.set_timing(True)
        ctx.reset_kernel_times()
        resident()
        ctx.synchronize()
        kernels = {name: round(ctx.kernel_time(name)[0], 4) for name in TIMERS}
        ctx.set_timing(False)
        out = {name: v.cpu().numpy() for name, v in out.items()}

        ex = sw.objects()
        real = out["top_frame"] >= 0
        ro = np.nonzero(real)[0].astype(np.int32)
        rf = out["top_frame"][real]
        scene = np.asarray(fr.scene_points, np.float32).astype(np.float64)
        host_in = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter()
            hb, hs, hi = ctx.proj_boxes(scene, ex["obj_pt_off"], ex["obj_pts"], k, w2c, W, H, ro, rf)
            host_in.append((time.perf_counter() - t0) * 1e3)
        host_in = host_in[1:]
        t0 = time.perf_counter()
        nb, ns, ni, fragile = R.boxes(scene, ex["obj_pt_off"], ex["obj_pts"], k, w2c, W, H, ro, rf)
        numpy_s = time.perf_counter() - t0
    same = bool(all(np.array_equal(x, y) and np.array_equal(x, z) for x, y, z in
                    ((out["boxes"][real], hb, nb), (out["status"][real], hs, ns), (out["inside"][real], hi, ni))))
    sizes = np.diff(ex["obj_pt_off"])
    nbytes = int(sizes[np.unique(ro)].sum()) * 28
    med = float(np.median(ms))
    res = {"what": f"projected boxes of the top {a.top_k} views of one {a.shape} scene: device-resident, host arrays in, numpy",
           "device": torch.cuda.get_device_name(0), "frames": [F, H, W], "objects": int(len(sizes)),
           "object_points": int(sizes.sum()), "requests": int(real.sum()), "padded": int((~real).sum()),
           "status_counts": np.bincount(ns, minlength=3).tolist(), "fragile": int(fragile.sum()),
           "resident_ms": dict(median=round(med, 4), min=round(min(ms), 4), max=round(max(ms), 4), repeats=a.repeats),
           "resident_kernels_ms": kernels, "algorithmic_bytes": nbytes,
           "resident_gbps": round(nbytes / (med * 1e-3) / 1e9, 2),
           "kernel_gbps": round(nbytes / (max(kernels["proj_boxes"], 1e-9) * 1e-3) / 1e9, 2),
           "host_in_ms": dict(median=round(float(np.median(host_in)), 3), min=round(min(host_in), 3),
                              max=round(max(host_in), 3), repeats=a.repeats),
           "numpy_s": round(numpy_s, 3), "numpy_over_resident": round(numpy_s * 1e3 / med, 1),
           "numpy_over_host_in": round(numpy_s * 1e3 / float(np.median(host_in)), 1), "all_routes_equal": same}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
