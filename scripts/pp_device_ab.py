"""Post-processing of one scene's clustered objects, two routes, in one process:
  (a) the drop-in route: the clustered nodes on the host -> post_process_objects (mc_pp_run behind
      it, CSR fast path) -> the reference's lists;
  (b) the device-resident route: mc_pp_run_clustered on the context's S1-S6 result + mc_pp_export to
      host arrays.
Wall time per call (median of --runs after 2 warm-up calls) and the pp_* timer totals per call of
each route.  Prints one JSON line.  GPU run: python scripts/pp_device_ab.py [--shape c2] [--b-only]"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from maskclustering_amd import _device  # noqa: E402
from maskclustering_amd._native import PPParams  # noqa: E402
from maskclustering_amd.synthetic_frames import make_frames_shape  # noqa: E402
from maskclustering_amd.utils import post_process as pp  # noqa: E402

TIMERS = ["pp_prep", "pp_dbscan", "pp_filter", "pp_merge", "pp_export"]


def timed(ctx, fn, runs):
    import torch
    wall = []
    for _ in range(runs + 2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t) * 1e3)
    ctx.set_timing(True)
    ctx.reset_kernel_times()
    for _ in range(5):
        fn()
    ctx.synchronize()
    timers = {k: round(ctx.kernel_time(k)[0] / 5, 4) for k in TIMERS}
    ctx.set_timing(False)
    return {"wall_ms_median": round(float(np.median(wall[2:])), 3), "wall_ms": [round(x, 2) for x in wall],
            "timers_ms_per_call": timers}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--runs", type=int, default=12)
    ap.add_argument("--b-only", action="store_true")
    a = ap.parse_args()
    fr = make_frames_shape(a.shape, seed=0, device="cuda:0")
    out = {"what": f"post-processing of one {a.shape} scene: (a) drop-in route, (b) device-resident route",
           "device": torch.cuda.get_device_name(0), "P": int(fr.num_points), "F": int(fr.num_frames)}
    if not a.b_only:
        from maskclustering_amd.graph import construction, iterative_clustering
        fids = [int(x) for x in np.arange(0, 10 * fr.num_frames, 10)]
        args = SimpleNamespace(debug=False, point_filter_threshold=0.5, **bench.CFG)
        ds = bench.FrameDataset(fr, fids, raw_depth=True)
        nodes, thr, mpc, pfm = construction.mask_graph_construction(args, fr.scene_points, fids, ds)
        objects = iterative_clustering.iterative_clustering(nodes, thr, args.view_consensus_threshold, False)
        res = []
        out["a"] = timed(_device.context(), lambda: res.append(
            pp.post_process_objects(objects, mpc, fr.scene_points, pfm, fids, 0.5)), a.runs)
        out["a"]["num_final"] = len(res[-1][0])
        del nodes, objects, mpc, pfm, res
    from maskclustering_amd.sweep import SceneSweep
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    sw = SceneSweep(0, bench.shape_thresholds(a.shape)[1], stream=torch.cuda.current_stream().cuda_stream)
    sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                 t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64))
    prm = PPParams(0.1, 4, 0.5, 0.8)
    res = []

    def route_b():
        sw.ctx.pp_run_clustered(prm)
        res.append(sw.ctx.pp_export())
    out["b"] = timed(sw.ctx, route_b, a.runs)
    i = sw.ctx.pp_info()
    out["b"].update(num_final=int(i.num_final), num_nodes=int(len(np.unique(res[-1]["obj_node"]))),
                    num_entries=int(i.num_entries), num_node_masks=int(i.num_node_masks))
    t0 = time.perf_counter()
    pm = sw.pred_masks(device=True)
    torch.cuda.synchronize()
    out["b"]["pred_masks_device_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
    out["b"]["pred_masks_shape"] = list(pm.shape)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
