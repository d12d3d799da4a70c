"""The AP table of a scene-parallel sweep on one rank, two routes, in one process.  The scenes are the
C2 sweep inputs of scripts/ap_device_ab.py (class-agnostic, slab ground truth), run once through
SceneSweep; scene i belongs to notional rank i mod 8, and every rank is a context of its own that
holds its scenes' scans (put there through mc_ev_add_matches, outside the timing).
  (a) state:  mc_ev_state_export on the 8 rank contexts, mc_ev_state_merge of the 8 buffers into a
              fresh context, mc_ev_ap there;
  (b) tables: the parent commit's only route: every scan's tables fetched with ev_scan() on its rank
              (timed where the scan is the rank's last one, as it is in a sweep), mc_ev_add_matches of
              every scan on a fresh context (the greedy pass again), mc_ev_ap there.
Every repeat rebuilds the rank contexts first (an export is cached until the accumulation changes), and
the two routes alternate in order.  No transport is timed: (a) ships state_bytes, (b) ships table_bytes.
Reported: wall time of each route over the repeats (median, min, max, ms) with (a) split into export /
merge / table, the bytes either route ships, the runs and examples, and whether the two tables (and the
one context that saw every scene) agree bit for bit.  Prints one JSON line.
GPU run: python scripts/ap_state_ab.py [--shape c2] [--seeds 16] [--repeats 9]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from maskclustering_amd import _native  # noqa: E402
from maskclustering_amd._native import PPParams  # noqa: E402
from maskclustering_amd.sweep import SceneSweep, scenes_of  # noqa: E402
from maskclustering_amd.synthetic_frames import make_frames_shape, slab_ground_truth  # noqa: E402

CLS = (3, 5, 8)
RANKS = 8


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--seeds", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
    sw = SceneSweep(0, bench.shape_thresholds(a.shape)[1], stream=torch.cuda.current_stream().cuda_stream)
    sw.begin_evaluation(CLS, no_class=True)
    prm = PPParams(0.1, 4, 0.5, 0.8)
    tables = []
    for seed in range(a.seeds):
        fr = make_frames_shape(a.shape, seed=seed)
        gt = slab_ground_truth(fr.scene_points, CLS)
        sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                     t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64), post_process=prm,
                     gt_ids=t(gt, torch.int32))
        tables.append(sw.ctx.ev_scan())
    whole_ap, whole_stats = sw.ctx.ev_ap()

    def fresh():
        ctx = _native.Context(0)
        ctx.ev_begin(CLS, None, 100, True)
        return ctx

    ranks, target_a, target_b = [fresh() for _ in range(RANKS)], fresh(), fresh()
    now = time.perf_counter
    rows = []
    for rep in range(a.warmup + a.repeats):
        fetch_ms = 0.0
        for r, ctx in enumerate(ranks):
            ctx.ev_begin(CLS, None, 100, True)
            for s in scenes_of(r, RANKS, a.seeds):
                ctx.ev_add_matches(tables[s])
                t0 = now()
                got = ctx.ev_scan()                       # (b)'s fetch of this scan on its rank
                fetch_ms += (now() - t0) * 1e3
            assert len(got["pr_cls"]) == len(tables[s]["pr_cls"])

        def route_a():
            target_a.ev_begin(CLS, None, 100, True)
            t0 = now()
            states = [ctx.ev_state() for ctx in ranks]
            t1 = now()
            for st in states:
                target_a.ev_merge_state(st)
            t2 = now()
            res = target_a.ev_ap()
            t3 = now()
            return res, states, [(x - y) * 1e3 for x, y in ((t1, t0), (t2, t1), (t3, t2), (t3, t0))]

        def route_b():
            target_b.ev_begin(CLS, None, 100, True)
            t0 = now()
            for r in range(RANKS):
                for s in scenes_of(r, RANKS, a.seeds):
                    target_b.ev_add_matches(tables[s])
            t1 = now()
            res = target_b.ev_ap()
            t2 = now()
            return res, [fetch_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3, fetch_ms + (t2 - t0) * 1e3]

        if rep % 2 == 0:
            (ap_a, st_a), states, ta = route_a()
            (ap_b, st_b), tb = route_b()
        else:
            (ap_b, st_b), tb = route_b()
            (ap_a, st_a), states, ta = route_a()
        if rep >= a.warmup:
            rows.append(dict(a_export=ta[0], a_merge=ta[1], a_table=ta[2], a_total=ta[3], b_fetch=tb[0], b_add_matches=tb[1],
                             b_table=tb[2], b_total=tb[3]))
    agree = bool(np.array_equal(ap_a, ap_b, equal_nan=True) and np.array_equal(st_a, st_b) and
                 np.array_equal(ap_a, whole_ap, equal_nan=True) and np.array_equal(st_a, whole_stats) and
                 ap_a.tobytes() == ap_b.tobytes() == whole_ap.tobytes())
    med = lambda k: dict(median=round(float(np.median([r[k] for r in rows])), 3),  # noqa: E731
                         min=round(min(r[k] for r in rows), 3), max=round(max(r[k] for r in rows), 3))
    info = [ctx.ev_state_info() for ctx in ranks]
    out = {"what": f"AP table of {a.seeds} {a.shape} scenes over {RANKS} notional ranks: state export/merge vs table replay",
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "warmup": a.warmup,
           "ms": {k: med(k) for k in rows[0]},
           "state_bytes": int(sum(len(s) for s in states)), "state_bytes_per_rank": [int(len(s)) for s in states],
           "table_bytes": int(sum(v.nbytes for tb_ in tables for v in tb_.values())),
           "runs": int(sum(i[0] for i in info)), "examples": int(sum(i[1] for i in info)),
           "scans": a.seeds, "pairs": int(sum(len(tb_["pair_int"]) for tb_ in tables)),
           "tables_agree_bit_for_bit": agree, "state_faster": bool(med("a_total")["median"] < med("b_total")["median"])}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
