"""Device-resident post-processing and export (mc_pp_run_device, mc_pp_run_clustered, mc_pp_export,
mc_pp_export_pred_masks) against mc_pp_run, the Python rebuild of the drop-in and the CPU
restatement (oracle/pp_oracle.py).  Bit-exact: info, every result array, point and mask lists,
coverages (float64), representative masks, the prediction matrix.

mc_pp_run uploads its arrays and takes the device entry's path (k_pp_validate, k_pp_prep, k_pp_order), so
the entry-against-entry tests below pin the upload; the independent check of those kernels is
test_gpu_pp.py, which compares mc_pp_run with the reference's goldens and the oracle, the
MC_PP_BIG_MIN=60 and MC_PP_GREEDY_CAP=0 cases included."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import pp_oracle
from pp_limit_inputs import pack_arrays as _pack_arrays
from test_gpu_pp import synthetic_pp

pytestmark = pytest.mark.gpu

RESULT_KEYS = ["entry_object", "mask_object", "mask_coverage", "object_state", "object_node", "object_bbox"]
THR = [0.5, 0.7, 0.2, 0.3]


def _pp():
    from maskclustering_amd.utils import post_process
    return post_process


@functools.lru_cache(maxsize=None)
def _ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


def _params(thr, eps=0.1):
    from maskclustering_amd._native import PPParams
    return PPParams(float(eps), 4, float(thr), 0.8)


@functools.lru_cache(maxsize=None)
def _packed(seed):
    """The mc_pp_run arguments of a synthetic_pp scene (mask table in mpc key order, points sorted),
    and the oracle's inputs for the same table."""
    scene, pfm, fids, mpc, nodes = synthetic_pp(seed, **(dict(nb=12, n_nodes=50) if seed == 3 else {}))
    keys = list(mpc.keys())
    kidx = {k: i for i, k in enumerate(keys)}
    col = {f: c for c, f in enumerate(fids)}
    mask_pts = [np.array(sorted(mpc[k]), np.int64) for k in keys]
    mask_col = np.array([col[int(k.rsplit("_", 1)[0])] for k in keys], np.int32)
    onodes = [([kidx[f"{f}_{m}"] for f, m in ml], np.asarray(vf, bool), np.asarray(pts, np.int64))
              for ml, vf, pts in nodes]
    return dict(scene=scene, pfm=pfm, fids=fids, mpc=mpc, nodes=nodes, keys=keys, mask_pts=mask_pts, mask_col=mask_col,
                onodes=onodes, args=_pack_arrays(scene, pfm, mask_pts, mask_col, onodes))


def _run_host(ctx, prm, a):
    ctx.pp_run(prm, a["scene"], a["pfm"], a["F"], a["moff"], a["mpts"], a["vf"], a["poff"], a["pts"], a["qoff"], a["qm"],
               a["qc"])


def _run_device(ctx, prm, a):
    import torch
    dev = ctx.torch_device

    def t(x):
        x = np.ascontiguousarray(x)
        return torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to(dev)
    ctx.pp_run_device(prm, t(a["scene"]), t(a["pfm"]), a["F"], t(a["moff"]), t(a["mpts"]), t(a["vf"]), t(a["poff"]),
                      t(a["pts"]), t(a["qoff"]), t(a["qm"]), t(a["qc"]))


def _info(ctx):
    i = ctx.pp_info()
    return (i.num_objects, i.num_filtered, i.num_final, i.num_entries, i.num_node_masks)


def _same_results(ctx, run_a, run_b):
    run_a()
    ia, ra = _info(ctx), ctx.pp_results()
    run_b()
    ib, rb = _info(ctx), ctx.pp_results()
    assert ia == ib
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(ra[k], rb[k], err_msg=k)
    return ia


# ---- 1. the device entry equals the host entry ------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_device_entry_equals_host_entry(seed):
    ctx, a, prm = _ctx(), _packed(seed)["args"], _params(THR[seed])
    info = _same_results(ctx, lambda: _run_host(ctx, prm, a), lambda: _run_device(ctx, prm, a))
    assert info[2] > 3 and info[1] > info[2]                         # objects filtered, objects merged away


def test_device_entry_split_dbscan_path(monkeypatch):
    monkeypatch.setenv("MC_PP_BIG_MIN", "60")
    ctx, a, prm = _ctx(), _packed(3)["args"], _params(0.5)
    _same_results(ctx, lambda: _run_host(ctx, prm, a), lambda: _run_device(ctx, prm, a))


def test_device_entry_device_greedy_merge(monkeypatch):
    monkeypatch.setenv("MC_PP_GREEDY_CAP", "0")
    ctx, a, prm = _ctx(), _packed(3)["args"], _params(0.5)
    _same_results(ctx, lambda: _run_host(ctx, prm, a), lambda: _run_device(ctx, prm, a))


# ---- 2. the export equals the Python rebuild and the oracle -------------------------------------
def _export_lists(r):
    po, mo = r["obj_pt_off"], r["obj_mask_off"]
    pts = [np.asarray(r["obj_pts"][po[k]:po[k + 1]], np.int64) for k in range(len(po) - 1)]
    masks = [[(int(m), float(c)) for m, c in zip(r["obj_masks"][mo[k]:mo[k + 1]], r["obj_mask_cov"][mo[k]:mo[k + 1]])]
             for k in range(len(mo) - 1)]
    return pts, masks


def _check_export(ctx, P, want_pts, want_masks):
    """pp_export (host and device outputs) and pp_pred_masks against lists of point ids and of
    (mask row, coverage); obj_repre against find_represent_mask.  Returns the host export."""
    r = ctx.pp_export()
    d = ctx.pp_export(device=True)
    assert set(r) == set(d)
    for k in r:
        np.testing.assert_array_equal(r[k], d[k].cpu().numpy(), err_msg=k)
    pts, masks = _export_lists(r)
    assert len(pts) == len(want_pts) == len(want_masks) == ctx.pp_info().num_final
    for k in range(len(pts)):
        np.testing.assert_array_equal(pts[k], np.asarray(want_pts[k], np.int64), err_msg=f"object {k}")
        assert masks[k] == [(int(m), float(c)) for m, c in want_masks[k]], f"object {k} masks"
        info = [(0, m, c) for m, c in masks[k]]                       # (frame, mask, coverage) as in mask_list
        rep = [info[i] for i in r["obj_repre"][k] if i >= 0]
        assert rep == _pp().find_represent_mask(list(info)), f"object {k} representative masks"
        assert (r["obj_repre"][k] >= 0).sum() == min(5, len(masks[k]))
    want = np.zeros((P, len(pts)), np.uint8)                          # export(): m[list(point_ids)] = True, stacked
    for k, p in enumerate(want_pts):
        want[np.asarray(p, np.int64), k] = 1
    pm = ctx.pp_pred_masks(P)
    assert pm.shape == want.shape and pm.dtype == np.uint8
    np.testing.assert_array_equal(pm, want)
    np.testing.assert_array_equal(ctx.pp_pred_masks(P, device=True).cpu().numpy(), want)
    return r


@pytest.mark.parametrize("seed", [0, 3])
def test_export_equals_rebuild_and_oracle(seed):
    from test_gpu_pp import _node
    ctx, z = _ctx(), _packed(seed)
    wp, wm = pp_oracle.post_process_objects(z["scene"], z["pfm"], z["mask_pts"], z["mask_col"], z["onodes"], THR[seed])
    assert len(wp) > 3
    _run_host(ctx, _params(THR[seed]), z["args"])
    r = _check_export(ctx, len(z["scene"]), wp, wm)
    np.testing.assert_array_equal(r["obj_node"], ctx.pp_results()["object_node"][ctx.pp_results()["object_state"] == 2])
    gp, gm = _pp().post_process_objects([_node(*n) for n in z["nodes"]], z["mpc"], z["scene"], z["pfm"], z["fids"], THR[seed])
    pts, masks = _export_lists(r)
    assert len(gp) == len(pts)
    for k in range(len(pts)):
        np.testing.assert_array_equal(gp[k], pts[k])
        key = lambda q: (int(z["keys"][q].rsplit("_", 1)[0]), int(z["keys"][q].rsplit("_", 1)[1]))  # noqa: E731
        assert gm[k] == [(*key(q), c) for q, c in masks[k]]


# ---- 3. the clustered entry, end to end -----------------------------------------------------------
SCENES = [("tiny", 2, 5), ("small", 0, 30), ("small", 1, 30)]
PRM = (0.1, 4, 0.5, 0.8)


@functools.lru_cache(maxsize=None)
def _sweep():
    import torch
    from maskclustering_amd.dataset_configs import graph_thresholds
    from maskclustering_amd.sweep import SceneSweep
    return SceneSweep(0, graph_thresholds("scannet"), stream=torch.cuda.current_stream().cuda_stream)


def _run_scene(shape, seed):
    """S1-S6 + device post-processing of one synthetic scene; (sweep, final count, float32 points)."""
    import torch
    from maskclustering_amd._native import PPParams
    from maskclustering_amd.synthetic_frames import make_frames_shape
    sw = _sweep()
    fr = make_frames_shape(shape, seed=seed)
    dev = torch.device("cuda", 0)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev, dt)  # noqa: E731
    n = sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                     t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64),
                     post_process=PPParams(*PRM))
    return sw, n, np.asarray(fr.scene_points, np.float32)


def _clustered_inputs(sw, pts32):
    """Nodes from run.canonical(dense=False) (ascending points, members as input mask rows) and the
    mask table / point-frame bits from the getters: the oracle's inputs and mc_pp_run's arguments."""
    from maskclustering_amd.pipeline import bits_to_bool
    got = sw.run.canonical(dense=False)
    P, F = sw.run.P, sw.run.F
    dcol, _, doff, dpts = sw.ctx.bp_masks()
    mask_pts = [np.asarray(dpts[doff[i]:doff[i + 1]], np.int64) for i in range(len(dcol))]
    pfm = bits_to_bool(sw.ctx.point_frame_bits(P, F), F)
    mo, po = got["obj_mask_off"], got["obj_pt_off"]
    rows = got["_input_index"][got["obj_mask_idx"]]
    vf = np.unpackbits(got["obj_vf_bits"], axis=1)[:, :F].astype(bool)
    onodes = [(rows[mo[k]:mo[k + 1]].tolist(), vf[k], np.asarray(got["obj_pt_idx"][po[k]:po[k + 1]], np.int64))
              for k in range(len(mo) - 1)]
    for _, _, p in onodes:
        assert (np.diff(p) > 0).all()
    scene = pts32.astype(np.float64)                                  # float32 widened exactly
    return scene, pfm, mask_pts, np.asarray(dcol, np.int32), onodes


@functools.lru_cache(maxsize=None)
def _oracle_scene(shape, seed):
    sw, n, pts32 = _run_scene(shape, seed)
    scene, pfm, mask_pts, mask_col, onodes = _clustered_inputs(sw, pts32)
    wp, wm = pp_oracle.post_process_objects(scene, pfm, mask_pts, mask_col, onodes, PRM[2], eps=PRM[0],
                                            min_points=PRM[1], overlapping_ratio=PRM[3])
    return wp, wm


@pytest.mark.parametrize("shape,seed,min_final", SCENES)
def test_clustered_entry_end_to_end(shape, seed, min_final):
    from maskclustering_amd._native import PPParams
    wp, wm = _oracle_scene(shape, seed)
    sw, n, pts32 = _run_scene(shape, seed)
    assert n == len(wp) == sw.ctx.pp_info().num_final and n >= min_final
    r = _check_export(sw.ctx, sw.run.P, wp, wm)
    for k, v in sw.objects().items():
        np.testing.assert_array_equal(v, r[k], err_msg=k)
    np.testing.assert_array_equal(sw.pred_masks(), sw.ctx.pp_pred_masks())
    assert tuple(sw.pred_masks(device=True).shape) == (sw.run.P, n)
    if shape == "small":                                              # the stable top-5 order is exercised
        mo = r["obj_mask_off"]
        tied = sum(len(set(r["obj_mask_cov"][mo[k]:mo[k + 1]].tolist())) < mo[k + 1] - mo[k] for k in range(n))
        assert tied >= 1
    # the same arrays through the host entry: info and every result array
    info, res = _info(sw.ctx), sw.ctx.pp_results()
    a = _pack_arrays(*_clustered_inputs(sw, pts32))
    _run_host(sw.ctx, PPParams(*PRM), a)
    assert _info(sw.ctx) == info
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(sw.ctx.pp_results()[k], res[k], err_msg=k)


# ---- 4. post_process_device + export ---------------------------------------------------------------
def test_post_process_device_and_export(tmp_path, monkeypatch):
    wp, wm = _oracle_scene("small", 0)
    sw, n, pts32 = _run_scene("small", 0)
    fids = [int(x) * 10 for x in range(sw.run.F)]
    got_pts, got_masks = _pp().post_process_device(sw.run, fids, PRM[2])
    col, lab = sw.run.mask_col, sw.run.mask_label
    want_masks = [[(fids[col[m]], int(lab[m]), c) for m, c in ml] for ml in wm]
    assert all(p.dtype == np.int64 for p in got_pts)
    out = {}
    for name, (pts, masks) in dict(got=(got_pts, got_masks), want=(wp, want_masks)).items():
        d = tmp_path / name
        d.mkdir()
        monkeypatch.chdir(d)
        ds = SimpleNamespace(get_scene_points=lambda: pts32, object_dict_dir=str(d / "object_dict"))
        _pp().export(ds, [np.asarray(p, np.int64) for p in pts], [list(m) for m in masks],
                     SimpleNamespace(config="cfg", seq_name="scene"))
        z = np.load(d / "data" / "prediction" / "cfg_class_agnostic" / "scene.npz")
        od = np.load(d / "object_dict" / "cfg" / "object_dict.npy", allow_pickle=True).item()
        out[name] = (z["pred_masks"], od)
    np.testing.assert_array_equal(out["got"][0], out["want"][0])
    assert out["got"][0].shape == (len(pts32), n)
    god, wod = out["got"][1], out["want"][1]
    assert list(god) == list(wod) == list(range(n))
    for k in range(n):
        np.testing.assert_array_equal(god[k]["point_ids"], wod[k]["point_ids"])
        assert god[k]["mask_list"] == wod[k]["mask_list"]
        assert god[k]["repre_mask_list"] == wod[k]["repre_mask_list"]


# ---- 5. states and errors -----------------------------------------------------------------------
def _small_args(qc=(0, 1), vf=(1, 1, 0, 0), pts=((0, 0, 0), (0.01, 0, 0), (0, 0.01, 0), (0.01, 0.01, 0), (5, 5, 5))):
    scene = np.array(pts, np.float64)
    P, F = len(scene), 4
    pfm = np.ones((P, F), bool)
    mask_pts = [np.arange(4, dtype=np.int64), np.arange(1, 4, dtype=np.int64)]
    onodes = [([0, 1], np.array(vf, bool), np.arange(P, dtype=np.int64))]
    return _pack_arrays(scene, pfm, mask_pts, np.array(qc, np.int32), onodes)


def test_states_and_errors():
    from maskclustering_amd import _native
    from maskclustering_amd.pipeline import GraphRun
    from maskclustering_amd.synthetic import make_shape
    ctx = _native.Context(0)
    with pytest.raises(_native.McError) as e:
        ctx.pp_run_clustered(_params(0.5))                            # before clustering
    assert e.value.code == _native.MC_ERR_STATE
    with pytest.raises(_native.McError) as e:
        ctx.pp_export()                                               # no result
    assert e.value.code == _native.MC_ERR_STATE
    run = GraphRun(0, ctx)
    sc = make_shape("c1", seed=0)
    run.set_scene(sc)
    run.step(mask_visible_threshold=0.3, undersegment_filter_threshold=0.3, view_consensus_threshold=0.9,
             contained_threshold=0.8)
    with pytest.raises(_native.McError) as e:
        ctx.pp_run_clustered(_params(0.5))                            # NULL scene, no points set
    assert e.value.code == _native.MC_ERR_STATE
    rng = np.random.default_rng(0)
    ctx.pp_run_clustered(_params(0.5), rng.uniform(0, 1, (sc.num_points, 3)))   # a host scene works
    assert ctx.pp_info().num_entries > 0

    ok = _small_args()
    _run_device(ctx, _params(0.0), ok)
    assert ctx.pp_info().num_final == 1 and ctx.pp_export()["obj_pts"].tolist() == [0, 1, 2, 3]

    def empty():
        r = ctx.pp_export()
        assert ctx.pp_info().num_final == 0
        assert r["obj_pt_off"].tolist() == [0] and r["obj_mask_off"].tolist() == [0]
        assert all(len(r[k]) == 0 for k in ("obj_pts", "obj_masks", "obj_mask_cov", "obj_node"))
        assert r["obj_repre"].shape == (0, 5)
        assert ctx.pp_pred_masks(5).shape == (5, 0) and tuple(ctx.pp_pred_masks(5, device=True).shape) == (5, 0)

    for run in (_run_device, _run_host):                                  # the same checks behind both entries
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0), _small_args(vf=(1, 0, 0, 0)))          # frame 1 not visible (:69)
        assert e.value.code == _native.MC_ERR_INVALID
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0, eps=1e-7), ok)                          # 5 / 1.01e-7 cells > 2^21
        assert e.value.code == _native.MC_ERR_UNSUPPORTED
        bad = dict(ok, pts=ok["pts"].copy())
        bad["pts"][2] = 5                                                 # node point out of [0, P)
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0), bad)
        assert e.value.code == _native.MC_ERR_INVALID
        bad = dict(ok, qm=np.array([0, 2], np.int32))                     # mask row out of the table
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0), bad)
        assert e.value.code == _native.MC_ERR_INVALID
        assert ok["moff"].tolist() == [0, 4, 7]
        bad = dict(ok, moff=np.array([0, 8, 7], np.int64))                # mask offsets: interior entry above the last
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0), bad)
        assert e.value.code == _native.MC_ERR_INVALID
        with pytest.raises(_native.McError) as e:
            ctx.pp_info()                                                 # the failed call left no result
        assert e.value.code == _native.MC_ERR_STATE
        run(ctx, _params(0.0), ok)                                        # a good call on the same context
        assert ctx.pp_info().num_final == 1 and ctx.pp_export()["obj_pts"].tolist() == [0, 1, 2, 3]

        none = dict(ok, vf=ok["vf"][:0], poff=ok["poff"][:1], pts=ok["pts"][:0], qoff=ok["qoff"][:1], qm=ok["qm"][:0],
                    qc=ok["qc"][:0])
        run(ctx, _params(0.0), none)                                      # empty node list
        assert ctx.pp_info().num_objects == 0
        empty()
        run(ctx, _params(1.0), ok)                                        # no ratio is above 1: every object filtered out
        assert ctx.pp_info().num_objects > 0
        empty()
