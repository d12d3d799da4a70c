"""AP evaluation of a sweep of scenes, two routes, in one process, every scene accumulated into one
evaluation (class-agnostic, slab ground truth of synthetic_frames.slab_ground_truth):
  (new)    mc_ev_add_scan_clustered per scene on the context's post-processed objects, mc_ev_ap at the end;
  (parent) pred_masks(device=False) -> mc_eval_match_counts on the dense [P, K] matrix -> the scan's
           match tables on the host -> tests/ap_restatement.py's greedy pass and AP loop (the stand-in
           for the reference's evaluate_matches).
Per scene the two routes alternate (even scenes new first, odd scenes parent first), after one warm-up
scene.  Reported: per-scene wall time of each route (median, min, max), the parent route's device-side
part alone (the pp_export + eval_counts timers: k_pp_ex_pred and k_eval_counts), the new route's kernel
timers, the final table's time on each route, and whether in every pair the new route's per-scene wall
time is below the parent's device-side part.  Prints one JSON line.
GPU run: python scripts/ap_device_ab.py [--shape c2] [--seeds 8]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import ap_restatement as R  # noqa: E402
import bench  # noqa: E402
from maskclustering_amd._native import PPParams  # noqa: E402
from maskclustering_amd.synthetic_frames import make_frames_shape, slab_ground_truth  # noqa: E402

CLS = (3, 5, 8)
NEW_TIMERS = ("ev_scan", "ev_greedy", "ev_ap")


def parent_tables(ctx, pm, gt, min_region=100):
    """The parent's route for one scan (--no_class): counts on the dense matrix, then the match tables."""
    ids = gt.astype(np.int64) % 1000 + CLS[0] * 1000
    uniq, cnt = np.unique(ids, return_counts=True)
    ginst = np.searchsorted(uniq, ids).astype(np.int32)          # every id is an instance of class 0
    verts, vint, inter = ctx.eval_match_counts(pm, ginst, len(uniq), np.zeros(len(ids), np.uint8))
    kept = np.flatnonzero(verts >= min_region)
    pp, pg = np.nonzero(inter[kept])
    return dict(gt_cls=np.zeros(len(uniq), np.int32), gt_id=uniq.astype(np.int32), gt_vert=cnt.astype(np.int64),
                pr_cls=np.zeros(len(kept), np.int32), pr_vert=verts[kept], pr_void=vint[kept],
                pr_score=np.ones(len(kept)), pair_pred=pp.astype(np.int32), pair_gt=pg.astype(np.int32),
                pair_int=inter[kept][pp, pg])


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--seeds", type=int, default=8)
    a = ap.parse_args()
    from maskclustering_amd.sweep import SceneSweep
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    sw = SceneSweep(0, bench.shape_thresholds(a.shape)[1], stream=torch.cuda.current_stream().cuda_stream)
    ctx = sw.ctx
    prm = PPParams(0.1, 4, 0.5, 0.8)
    rs = R.APRestatement(CLS, None, 100, True)
    rows = []
    sync = torch.cuda.synchronize

    def scene(seed):
        fr = make_frames_shape(a.shape, seed=seed)
        gt = slab_ground_truth(fr.scene_points, CLS)
        n = sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                         t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64), post_process=prm)
        sw.objects(device=True)                  # the export arrays both routes read, built outside the timing
        return gt, t(gt, torch.int32), n, int(fr.num_points)

    def new_route(gt_dev):
        sync()
        t0 = time.perf_counter()
        ctx.ev_add_scan_clustered(gt_dev)
        sync()
        return (time.perf_counter() - t0) * 1e3

    def parent_route(gt, accumulate):
        sync()
        t0 = time.perf_counter()
        tab = parent_tables(ctx, sw.pred_masks(device=False), gt)
        t1 = time.perf_counter()
        if accumulate:
            rs.add_tables(tab)                   # the greedy pass in Python (part of evaluate_matches)
        return (t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3

    ctx.set_timing(True)
    sw.begin_evaluation(CLS, no_class=True)
    gt, gt_dev, _, _ = scene(10_000)             # warm-up: buffers sized, nothing kept
    new_route(gt_dev)
    parent_route(gt, False)
    sw.begin_evaluation(CLS, no_class=True)
    for seed in range(a.seeds):
        gt, gt_dev, n, P = scene(seed)
        ctx.reset_kernel_times()
        if seed % 2 == 0:
            new_ms = new_route(gt_dev)
            par_ms, greedy_ms = parent_route(gt, True)
        else:
            par_ms, greedy_ms = parent_route(gt, True)
            new_ms = new_route(gt_dev)
        ctx.synchronize()
        dev_ms = ctx.kernel_time("pp_export")[0] + ctx.kernel_time("eval_counts")[0]
        tab = ctx.ev_scan()
        rows.append(dict(seed=seed, P=P, K=int(n), kept=len(tab["pr_cls"]), instances=len(tab["gt_id"]),
                         pairs=len(tab["pair_int"]), new_ms=round(new_ms, 3), parent_ms=round(par_ms, 3),
                         parent_device_ms=round(dev_ms, 3), parent_greedy_py_ms=round(greedy_ms, 1),
                         new_kernels_ms={k: round(ctx.kernel_time(k)[0], 4) for k in NEW_TIMERS[:2]}))
    ctx.reset_kernel_times()
    sync()
    t0 = time.perf_counter()
    ev = sw.evaluation()
    ap_new_ms = (time.perf_counter() - t0) * 1e3
    ctx.synchronize()
    ap_kernel_ms = ctx.kernel_time("ev_ap")[0]
    t0 = time.perf_counter()
    want_ap, want_stats, curves = rs.result()
    ap_py_ms = (time.perf_counter() - t0) * 1e3
    n = np.ones_like(want_ap)
    for (c, o), cv in curves.items():
        n[c, o] = len(cv[0]) + 1
    col = lambda k: [r[k] for r in rows]  # noqa: E731
    med = lambda k: dict(median=round(float(np.median(col(k))), 3), min=min(col(k)), max=max(col(k)))  # noqa: E731
    out = {"what": f"AP evaluation of {a.seeds} {a.shape} scenes: new device route vs the parent's dense route",
           "device": torch.cuda.get_device_name(0), "scenes": rows,
           "per_scene_new_ms": med("new_ms"), "per_scene_parent_ms": med("parent_ms"),
           "per_scene_parent_device_ms": med("parent_device_ms"), "per_scene_parent_greedy_py_ms": med("parent_greedy_py_ms"),
           "new_below_parent_device_part_in_every_pair": bool(all(r["new_ms"] < r["parent_device_ms"] for r in rows)),
           "final_table_new_ms": round(ap_new_ms, 3), "final_table_new_kernel_ms": round(ap_kernel_ms, 4),
           "final_table_parent_py_ms": round(ap_py_ms, 1),
           "routes_agree": bool(np.array_equal(ev["stats"], want_stats) and R.ap_close(ev["ap"], want_ap, n)),
           "all_ap": float(ev["all_ap"]), "all_ap_50%": float(ev["all_ap_50%"]), "all_ap_25%": float(ev["all_ap_25%"])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
