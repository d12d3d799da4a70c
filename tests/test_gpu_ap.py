"""Device-resident AP evaluation (mc_ev_*) against the reference's own
evaluate_matches on tests/golden/ap_small.npz and against tests/ap_restatement.py.

AP entries: nan where the reference's are, exactly 0 where the reference's are, otherwise within
n * 2^-52 absolute (n = the cell's precision/recall points; derived in tests/test_ap_cpu.py).
Integers (scan tables, stats, curves) are exact."""
import functools
import json
import os
import re

import numpy as np
import pytest

import ap_restatement as R
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

MODES = ("ca", "nc")


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "ap_small.npz"))


@functools.lru_cache(maxsize=None)
def labels():
    return [str(x) for x in golden()["class_labels"]]


@functools.lru_cache(maxsize=None)
def caps():
    """(kEvInstCap, kEvSortCap): the tier limits the kernels state."""
    src = open(os.path.join(REPO, "maskclustering_amd", "csrc", "mc_ap_kernels.inl")).read()
    return tuple(int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("kEvInstCap", "kEvSortCap"))


@functools.lru_cache(maxsize=None)
def restated(mode, nscans):
    z = golden()
    rs = R.APRestatement(z["class_ids"], z["overlaps"], int(z["min_region_size"]), mode == "nc")
    for s in range(nscans):
        rs.add_scan(z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"])
    return rs.result()


def ref_dicts(mode, s):
    z = golden()
    return json.loads(str(z[f"{mode}_s{s}_gt2pred"])), json.loads(str(z[f"{mode}_s{s}_pred2gt"]))


def new_ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def begin_golden(ctx, mode):
    z = golden()
    ctx.ev_begin(z["class_ids"], z["overlaps"], int(z["min_region_size"]), mode == "nc")


def npoints(shape, curves):
    n = np.ones(shape)
    for (c, o), cv in curves.items():
        n[c, o] = len(cv[0]) + 1
    return n


def check_result(ctx, want_ap, rs_result, msg=""):
    """ev_ap against want_ap within the bound; stats and every curve against the restatement's, exactly."""
    rap, rstats, rcurves = rs_result
    ap, stats = ctx.ev_ap()
    np.testing.assert_array_equal(stats, rstats, err_msg=f"{msg} stats")
    assert R.ap_close(ap, want_ap, npoints(ap.shape, rcurves)), f"{msg} ap"
    C, O = ap.shape
    with_curve = 0
    for c in range(C):
        if not stats[c, :, 0].any():
            continue
        for o in range(O):
            got = ctx.ev_curve(c, o)
            if (c, o) in rcurves:
                with_curve += 1
                for a, b, k in zip(got, rcurves[(c, o)], ("score", "tp", "fp", "fn")):
                    np.testing.assert_array_equal(a, b, err_msg=f"{msg} cell {c},{o} {k}")
            else:
                assert len(got[0]) == 0
    assert with_curve == len(rcurves)
    return ap, stats


# ---- 1. ev_add_matches on the reference's own match dicts -----------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_add_matches_on_the_reference_dicts(mode):
    from maskclustering_amd.evaluation.evaluate import pack_matches
    z = golden()
    ctx = new_ctx()
    begin_golden(ctx, mode)
    for s in range(int(z["num_scans"])):
        ctx.ev_add_matches(pack_matches(*ref_dicts(mode, s), labels()))
    check_result(ctx, z[f"{mode}_ap"][0], restated(mode, 4), mode)


# ---- 2. ev_add_scan on the fixture's inputs --------------------------------------------------------
@pytest.mark.parametrize("device", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("mode", MODES)
def test_add_scan_on_the_fixture(mode, device):
    import torch
    z = golden()
    ctx = new_ctx()
    begin_golden(ctx, mode)
    for s in range(int(z["num_scans"])):
        args = [z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"]]
        if device:
            args = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for a in args]
        ctx.ev_add_scan(*args)
        R.assert_tables_equal(ctx.ev_scan(), R.tables_from_dicts(*ref_dicts(mode, s), labels()), f"{mode} scan {s}")
        if s == 1:      # mid-accumulation: the reference of two scans is the restatement, itself equal to the reference
            check_result(ctx, restated(mode, 2)[0], restated(mode, 2), f"{mode} after two scans")
    check_result(ctx, z[f"{mode}_ap"][0], restated(mode, 4), mode)


# ---- 3. equivalence with mc_eval_match_counts on the dense matrix ----------------------------------
def test_pairs_equal_the_dense_route():
    z = golden()
    ctx = new_ctx()
    begin_golden(ctx, "ca")
    s = 0
    gt, off, pts, classes = z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"]
    ctx.ev_add_scan(gt, off, pts, classes, z[f"s{s}_scores"])
    t = ctx.ev_scan()
    P, K, G = len(gt), len(off) - 1, len(t["gt_id"])
    dense = np.zeros((P, K), np.uint8)
    for k in range(K):
        dense[pts[off[k]:off[k + 1]], k] = 1
    ginst = np.full(P, -1, np.int32)
    for g, iid in enumerate(t["gt_id"]):
        ginst[gt == iid] = g
    void = ~np.isin(gt // 1000, z["class_ids"])
    verts, vint, inter = ctx.eval_match_counts(dense, ginst, G, void)
    cidx = {int(c): i for i, c in enumerate(z["class_ids"])}
    kept = [k for k in range(K) if int(classes[k]) in cidx and verts[k] >= int(z["min_region_size"])]
    np.testing.assert_array_equal(t["pr_vert"], verts[kept])
    np.testing.assert_array_equal(t["pr_void"], vint[kept])
    pairs = [(j, g, int(inter[k, g])) for j, k in enumerate(kept) for g in np.flatnonzero(inter[k])
             if t["gt_cls"][g] == cidx[int(classes[k])]]
    assert pairs and pairs == list(zip(t["pair_pred"].tolist(), t["pair_gt"].tolist(), t["pair_int"].tolist()))


# ---- 4. tier edges, against the restatement --------------------------------------------------------
CLS = (3, 5, 8)


def check_scans(scans, min_region=100, no_class=False, overlaps=None, tables=False):
    """scans: (gt, off, pts, classes, scores) each, or table dicts: the device against the restatement."""
    ctx = new_ctx()
    ctx.ev_begin(CLS, overlaps, min_region, no_class)
    rs = R.APRestatement(CLS, overlaps, min_region, no_class)
    for i, sc in enumerate(scans):
        if tables:
            ctx.ev_add_matches(sc)
            rs.add_tables(sc)
        else:
            ctx.ev_add_scan(*sc)
            R.assert_tables_equal(ctx.ev_scan(), rs.add_scan(*sc), f"scan {i}")
    res = rs.result()
    ap, stats = check_result(ctx, res[0], res)
    return ap, stats, rs


def lists(*ranges):
    off = np.concatenate([[0], np.cumsum([len(r) for r in ranges])]).astype(np.int64)
    pts = np.concatenate([np.asarray(r, np.int32) for r in ranges]) if ranges else np.zeros(0, np.int32)
    return off, pts


def test_prediction_touching_more_instances_than_the_lds_table():
    n = caps()[0] + 1                                   # instances of 2 points, all of one class
    assert n <= 999
    gt = np.repeat(CLS[1] * 1000 + 1 + np.arange(n), 2).astype(np.int32)
    off, pts = lists(np.arange(2 * n), np.arange(0, 2 * n, 2), np.arange(2 * n - 40, 2 * n))
    ap, stats, rs = check_scans([(gt, off, pts, np.array([CLS[1]] * 3, np.int32), np.array([0.9, 0.5, 0.7]))], min_region=1)
    assert stats[1, 0, 0] > 0


@pytest.mark.parametrize("scores", ("distinct", "equal"))
def test_cell_with_one_more_example_than_the_lds_sort(scores):
    n, ngt = caps()[1] + 1, 40
    rng = np.random.default_rng(5)
    # ngt instances each matched by one prediction (overlap 1), one of them by two; the rest plain false positives
    K = n                                               # every prediction gives one example per overlap
    sc = rng.permutation(K).astype(np.float64) / K if scores == "distinct" else np.ones(K)
    t = dict(gt_cls=np.full(ngt, 1, np.int32), gt_id=(CLS[1] * 1000 + 1 + np.arange(ngt)).astype(np.int32),
             gt_vert=np.full(ngt, 150, np.int64), pr_cls=np.full(K, 1, np.int32), pr_vert=np.full(K, 150, np.int64),
             pr_void=np.zeros(K, np.int64), pr_score=sc,
             pair_pred=np.r_[np.arange(ngt), ngt].astype(np.int32), pair_gt=np.r_[np.arange(ngt), 0].astype(np.int32),
             pair_int=np.full(ngt + 1, 150, np.int64))
    ap, stats, rs = check_scans([t], tables=True)
    assert (stats[1, :, 0] == n).all() and rs.counters["second_match"] == 10
    assert 0 < ap[1, 0] < 1 or scores == "equal"


def test_small_and_empty_scans():
    P = 900
    gt = np.zeros(P, np.int32)
    gt[:300] = CLS[0] * 1000 + 1
    gt[300:500] = CLS[2] * 1000 + 2
    gt[500:560] = CLS[2] * 1000 + 3                      # a too-small instance
    gt[600:700] = 999 * 1000 + 4                         # void
    none = lists()
    one = lists(np.arange(0, 280))
    c = lambda *x: np.array(x, np.int32)                 # noqa: E731
    f = lambda *x: np.array(x, np.float64)               # noqa: E731
    scans = [(gt, *none, c(), f()),                                         # zero predictions
             (np.zeros(P, np.int32), *one, c(CLS[0]), f(0.5)),             # zero instances
             (gt, *one, c(CLS[0]), f(0.8)),                                 # K = 1
             (gt, *lists(np.arange(300, 399), np.arange(300, 400), np.arange(500, 700)), c(CLS[2], CLS[2], CLS[2]),
              f(0.3, 0.6, 0.9))]                                            # min_region_size - 1 and min_region_size points
    for no_class in (False, True):
        ap, stats, rs = check_scans(scans, no_class=no_class)
        assert rs.counters["dropped_pred"] == 1 and (no_class or rs.counters["ignored_pred"] >= 1)


def test_overlap_equal_to_a_threshold_is_no_match():
    P = 700
    gt = np.zeros(P, np.int32)
    gt[:200] = CLS[0] * 1000 + 1                          # 100 of 200: 100 / (200 + 100 - 100) = 0.5
    gt[200:600] = CLS[0] * 1000 + 2                       # 100 of 400: 100 / (400 + 100 - 100) = 0.25
    off, pts = lists(np.arange(0, 100), np.arange(200, 300))
    ap, stats, rs = check_scans([(gt, off, pts, np.array([CLS[0]] * 2, np.int32), np.array([0.9, 0.8]))])
    ov = R.default_overlaps()
    i50, i25 = int(np.flatnonzero(ov == 0.5)[0]), int(np.flatnonzero(ov == 0.25)[0])
    # at 0.25 only the first prediction matches (0.5 > 0.25; 0.25 > 0.25 is false); at 0.5 none does
    assert stats[0, i25, 1] == 1 and stats[0, i25, 2] == 1
    assert stats[0, i50, 1] == 0 and stats[0, i50, 2] == 2


# ---- 5. the sweep route ----------------------------------------------------------------------------
SCENES = (("small", 0), ("small", 1), ("tiny", 2))
PRM = (0.1, 4, 0.5, 0.8)


def _sweep():
    import torch
    from maskclustering_amd.dataset_configs import graph_thresholds
    from maskclustering_amd.sweep import SceneSweep
    return SceneSweep(0, graph_thresholds("scannet"), stream=torch.cuda.current_stream().cuda_stream)


def _run(sw, fr, gt=None):
    import torch
    from maskclustering_amd._native import PPParams
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0", dt)  # noqa: E731
    return sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                        t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64),
                        post_process=PPParams(*PRM), gt_ids=None if gt is None else t(gt, torch.int32))


def test_sweep_evaluation():
    from maskclustering_amd.synthetic_frames import make_frames_shape, slab_ground_truth
    frames = [make_frames_shape(shape, seed=seed) for shape, seed in SCENES]
    gts = [slab_ground_truth(fr.scene_points, CLS) for fr in frames]
    a, b = _sweep(), _sweep()
    rs = {nc: R.APRestatement(CLS, None, 100, nc) for nc in (True, False)}
    a.begin_evaluation(CLS, no_class=True)
    b.begin_evaluation(CLS, no_class=False)
    kept = 0
    for fr, gt in zip(frames, gts):
        assert len(np.unique(gt)) > 4
        _run(a, fr, gt)                                   # adds the scene (mc_ev_add_scan_clustered, device ids)
        obj = a.objects()
        for nc in rs:
            t = rs[nc].add_scan(gt, obj["obj_pt_off"], obj["obj_pts"])
            if nc:
                R.assert_tables_equal(a.ctx.ev_scan(), t, "sweep scan")
                kept += len(t["pr_cls"])
        _run(b, fr)
        b.ctx.ev_add_scan_clustered(gt)                   # host ids, class-aware: class 0 is not in the table
        assert len(b.ctx.ev_scan()["pr_cls"]) == 0
    assert kept > 0
    res = rs[True].result()
    check_result(a.ctx, res[0], res, "sweep no_class")
    ev = a.evaluation()
    assert set(ev) >= {"ap", "all_ap", "all_ap_50%", "all_ap_25%", "classes"} and ev["ap"].shape == (3, 10)
    mine = R.compute_averages(ev["ap"], R.default_overlaps(), [str(c) for c in CLS])
    for k in ("all_ap", "all_ap_50%", "all_ap_25%"):
        assert ev[k] == mine[k]
    assert np.isfinite(ev["all_ap"])
    res = rs[False].result()
    ap_b, stats_b = check_result(b.ctx, res[0], res, "sweep class-aware")
    assert np.all((ap_b == 0) | np.isnan(ap_b)) and np.any(ap_b == 0)
    # the second context again, class-agnostic: the same table as the first
    b.begin_evaluation(CLS, no_class=True)
    for fr, gt in zip(frames, gts):
        _run(b, fr)
        b.ctx.ev_add_scan_clustered(gt)
    ap2, stats2 = b.ctx.ev_ap()
    np.testing.assert_array_equal(stats2, ev["stats"])
    np.testing.assert_array_equal(ap2, ev["ap"])


# ---- 6. errors leave the accumulation as it was ----------------------------------------------------
def test_errors():
    from maskclustering_amd._native import McError
    z = golden()
    scan = lambda s: [z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"]]  # noqa: E731
    ctx = new_ctx()
    with pytest.raises(McError):
        ctx.ev_add_scan(*scan(0))                         # before ev_begin
    begin_golden(ctx, "ca")
    ctx.ev_add_scan(*scan(0))
    gt, off, pts, cls, sc = scan(1)
    bad = pts.copy()
    bad[7] = len(gt)
    with pytest.raises(McError, match="point id"):
        ctx.ev_add_scan(gt, off, bad, cls, sc)
    bad = gt.copy()
    bad[11] = -1
    with pytest.raises(McError, match="negative"):
        ctx.ev_add_scan(bad, off, pts, cls, sc)
    bad = off.copy()
    bad[3] = bad[2] - 1
    with pytest.raises(McError, match="offsets"):
        ctx.ev_add_scan(gt, bad, pts, cls, sc)
    with pytest.raises(McError, match="post-processing"):
        ctx.ev_add_scan_clustered(gt)
    ctx.ev_add_scan(gt, off, pts, cls, sc)
    fresh = new_ctx()
    begin_golden(fresh, "ca")
    fresh.ev_add_scan(*scan(0))
    fresh.ev_add_scan(*scan(1))
    for x, y in zip(ctx.ev_ap(), fresh.ev_ap()):
        np.testing.assert_array_equal(x, y)
    check_result(ctx, restated("ca", 2)[0], restated("ca", 2), "after errors")


def worked_tables():
    """The worked scan of scripts/ap_plan_check.cpp: class index 0 has instances 0 and 1 (a group id) and
    predictions 0 and 1, class index 1 prediction 2 alone, class index 2 instances 2 and 3 (below
    min_region_size) alone; the four pairs are listed shuffled."""
    return dict(gt_cls=np.array([0, 0, 2, 2], np.int32), gt_id=np.array([3001, 500, 8002, 8003], np.int32),
                gt_vert=np.array([300, 200, 150, 60], np.int64), pr_cls=np.array([0, 0, 1], np.int32),
                pr_vert=np.array([280, 120, 90], np.int64), pr_void=np.array([10, 0, 5], np.int64),
                pr_score=np.array([0.9, 0.4, 0.7], np.float64), pair_pred=np.array([1, 1, 0, 0], np.int32),
                pair_gt=np.array([1, 0, 1, 0], np.int32), pair_int=np.array([20, 90, 15, 250], np.int64))


def test_rejected_tables_leave_the_accumulation():
    """The eleven table rules of mc_ev_add_matches, each broken alone on the worked scan: MC_ERR_INVALID with
    the rule's message, and the table, the stats and the last scan stay bit for bit what they were."""
    from maskclustering_amd._native import McError
    good = worked_tables()
    broken = (("gt_cls", 3, 3, "ascending class"),        # no class index
              ("gt_cls", 0, 2, "ascending class"),        # descending
              ("gt_vert", 2, 0, "vert_count"),
              ("pr_cls", 1, -1, "class index"),
              ("pr_vert", 0, 0, "prediction counts"),
              ("pr_void", 2, 91, "prediction counts"),    # more void than vertices
              ("pr_score", 1, np.nan, "NaN"),
              ("pair_pred", 0, 3, "pair index"),
              ("pair_gt", 2, -1, "pair index"),
              ("pair_gt", 0, 2, "across classes"),        # prediction 1 of class index 0, instance 2 of class index 2
              ("pair_int", 3, 281, "intersection"))       # above the prediction's 280 vertices
    ctx = new_ctx()
    ctx.ev_begin(CLS, None, 100, False)
    ctx.ev_add_matches(good)
    ap, stats = ctx.ev_ap()
    last = ctx.ev_scan()
    R.assert_tables_equal(last, good, "the worked scan")
    assert stats[:, :, 0].sum() > 0
    for key, i, v, fragment in broken:
        t = {k: a.copy() for k, a in good.items()}
        t[key][i] = v
        with pytest.raises(McError, match=fragment) as e:
            ctx.ev_add_matches(t)
        assert e.value.code == 1, f"{key}[{i}] = {v}: {e.value}"
        ap2, stats2 = ctx.ev_ap()
        assert ap2.tobytes() == ap.tobytes() and stats2.tobytes() == stats.tobytes(), f"{key}[{i}] = {v}"
        R.assert_tables_equal(ctx.ev_scan(), last, f"last scan after {key}[{i}] = {v}")
    ctx.ev_add_matches(good)                              # and the valid table still adds
    twice = new_ctx()
    twice.ev_begin(CLS, None, 100, False)
    twice.ev_add_matches(good)
    twice.ev_add_matches(good)
    for x, y in zip(ctx.ev_ap(), twice.ev_ap()):
        assert x.tobytes() == y.tobytes()
    assert (ctx.ev_ap()[1][:, :, 0] == 2 * stats[:, :, 0]).all()
