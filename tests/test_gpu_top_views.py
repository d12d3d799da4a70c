"""The projected boxes on the device (mc_proj_boxes, mc_proj_top_views, maskclustering_amd.top_images,
SceneSweep.top_views) against the fixture made by the reference's own get_top_images.py
(tests/golden/make_top_views_golden.py) and the numpy restatement (tests/top_views_restatement.py).

Against the reference: exact on the edge set; on the scene set exact on every request the
restatement does not flag FRAGILE (the dot product's summation order could decide it), at most 1 %
of them.  Against the restatement: boxes, status and in-bounds counts bit for bit on every request,
since both use the same operation order."""
import ctypes
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest

import top_views_restatement as R
from conftest import GOLDEN
from test_top_views_cpu import FRAGILE_CAP, scene_restatement

pytestmark = pytest.mark.gpu

PRM = (0.1, 4, 0.5, 0.8)


@functools.lru_cache(maxsize=None)
def _ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@functools.lru_cache(maxsize=None)
def _gold():
    return dict(np.load(os.path.join(GOLDEN, "top_views.npz")))


@functools.lru_cache(maxsize=None)
def _scene_want():
    return scene_restatement(_gold())


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device("cuda", 0), getattr(torch, dt))


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _call(ctx, points, off, ids, k, w2c, W, H, ro, rf, arrays, device_out=False):
    """proj_boxes with host arrays or the same arrays as device tensors; numpy results"""
    if arrays == "device":
        args = (_dev(points, "float64"), _dev(off, "int64"), _dev(ids, "int32"), _dev(k, "float64"), _dev(w2c, "float64"), W, H,
                _dev(ro, "int32"), _dev(rf, "int32"))
    else:
        args = (points, off, ids, k, w2c, W, H, ro, rf)
    return tuple(_np(a) for a in ctx.proj_boxes(*args, device=device_out))


@pytest.mark.parametrize("arrays,device_out", [("host", False), ("device", False), ("device", True), ("host", True)])
def test_scene_set_equals_fixture_and_restatement(arrays, device_out):
    z, ctx = _gold(), _ctx()
    wbox, wst, wins, fragile = _scene_want()
    assert fragile.mean() <= FRAGILE_CAP
    w2c = np.stack([np.linalg.inv(e) for e in z["extrinsics"]])
    for s in range(2):
        W, H = (int(v) for v in z["sizes"][s])
        box, st, ins = _call(ctx, z["points"], z["obj_pt_off"], z["obj_pts"], z["intrinsics"][s], w2c, W, H, z["requests"][:, 0],
                             z["requests"][:, 1], arrays, device_out)
        np.testing.assert_array_equal(st, wst[s])                         # the restatement: every request, bit for bit
        np.testing.assert_array_equal(box, wbox[s])
        np.testing.assert_array_equal(ins, wins[s])
        keep = ~fragile[s]                                                # the reference: every request that is not fragile
        np.testing.assert_array_equal(st[keep], z["status"][s][keep])
        np.testing.assert_array_equal(box[keep], z["boxes"][s][keep])


@pytest.mark.parametrize("arrays", ["host", "device"])
def test_edge_set_equals_reference_exactly(arrays):
    z, ctx = _gold(), _ctx()
    n = len(z["edge_name"])
    with np.errstate(all="ignore"):
        w2c = np.stack([np.linalg.inv(e) for e in z["edge_ext"]])          # one frame per case
    k = np.tile(z["edge_intrinsics"], (n, 1))
    off = np.concatenate([[0], np.cumsum(z["edge_npts"])]).astype(np.int64)
    points = np.concatenate([z["edge_pts"][j][:z["edge_npts"][j]] for j in range(n)])
    ids = np.arange(len(points), dtype=np.int32)
    sizes = sorted({tuple(int(v) for v in s) for s in z["edge_size"]})
    assert len(sizes) >= 5
    for W, H in sizes:                                                     # the image size is one per call
        sel = np.array([j for j in range(n) if tuple(z["edge_size"][j]) == (W, H)], np.int32)
        box, st, ins = _call(ctx, points, off, ids, k, w2c, W, H, sel, sel, arrays)
        for i, j in enumerate(sel):
            assert st[i] == z["edge_status"][j] and list(box[i]) == list(z["edge_box"][j]), (z["edge_name"][j], st[i], box[i])
            assert ins[i] == R.project(points[off[j]:off[j + 1]], w2c[j], k[j], W, H)[2], z["edge_name"][j]


def test_split_object_and_request_groups():
    """an object of several turns (kProjChunk = 4096 points each): its workgroups combine with atomics;
    more than 16 requests of one object: several groups"""
    ctx = _ctx()
    rng = np.random.default_rng(3)
    n_big, F, W, H = 3 * 4096 + 17, 20, 131, 97
    points = np.concatenate([rng.normal(0, 1.2, (n_big, 3)), rng.normal(0, 0.1, (300, 3))])
    off = np.array([0, 300, 300 + n_big], np.int64)                       # a small object first, the split one second
    ids = np.concatenate([np.arange(n_big, n_big + 300), rng.permutation(n_big)]).astype(np.int32)
    z = _gold()
    w2c = np.stack([np.linalg.inv(z["extrinsics"][f % 6]) for f in range(F)])
    w2c[6:, :3, 3] += rng.normal(0, 0.3, (F - 6, 3))
    k = np.tile(z["intrinsics"][0, 0], (F, 1))
    ro = np.array([1] * F + [0, 1, 1, 0], np.int32)                        # 22 requests of object 1, duplicates among them
    rf = np.array(list(range(F)) + [3, 3, 19, 0], np.int32)
    wbox, wst, wins, _ = R.boxes(points, off, ids, k, w2c, W, H, ro, rf)
    assert (wst == R.OK).sum() >= 10 and wins.max() > 4096
    for arrays in ("host", "device"):
        box, st, ins = _call(ctx, points, off, ids, k, w2c, W, H, ro, rf, arrays)
        np.testing.assert_array_equal(st, wst)
        np.testing.assert_array_equal(box, wbox)
        np.testing.assert_array_equal(ins, wins)
    for j in (0, 7, 19, 21):                                               # the same object, one request per call
        box, st, ins = _call(ctx, points, off, ids, k, w2c, W, H, ro[j:j + 1], rf[j:j + 1], "host")
        assert (st[0], list(box[0]), ins[0]) == (wst[j], list(wbox[j]), wins[j])


@functools.lru_cache(maxsize=None)
def _tiny():
    """S1-S6 + device post-processing of the tiny synthetic scene: (sweep, frames, W, H)"""
    import torch
    from maskclustering_amd._native import PPParams
    from maskclustering_amd.dataset_configs import graph_thresholds
    from maskclustering_amd.sweep import SceneSweep
    from maskclustering_amd.synthetic_frames import make_frames_shape
    sw = SceneSweep(0, graph_thresholds("scannet"), stream=torch.cuda.current_stream().cuda_stream)
    fr = make_frames_shape("tiny", seed=2)
    t = lambda a, dt: _dev(a, dt)  # noqa: E731
    n = sw.run_scene(t(fr.scene_points, "float32"), t(fr.depth, "float32"), t(fr.seg, "uint8"), t(fr.intrinsics, "float64"),
                     t(fr.poses.reshape(-1, 16), "float64"), post_process=PPParams(*PRM))
    assert n >= 5
    H, W = fr.depth.shape[1:]
    return sw, fr, int(W), int(H)


@pytest.mark.parametrize("top_k", [1, 9, 16])
@pytest.mark.parametrize("device", [False, True])
def test_top_views_equal_proj_boxes_on_the_export(top_k, device):
    sw, fr, W, H = _tiny()
    ctx = sw.ctx
    ex = ctx.pp_export()
    nf = len(ex["obj_pt_off"]) - 1
    k = np.asarray(fr.intrinsics, np.float64).reshape(-1, 4)
    w2c = np.linalg.inv(np.asarray(fr.poses, np.float64).reshape(-1, 4, 4))
    if device:
        out = ctx.proj_top_views(_dev(k, "float64"), _dev(w2c, "float64"), W, H, top_k=top_k, device=True)
    else:
        out = ctx.proj_top_views(k, w2c, W, H, top_k=top_k)
    out = {name: _np(v) for name, v in out.items()}
    np.testing.assert_array_equal(ctx.pp_export()["obj_repre"], ex["obj_repre"])           # unchanged by the call
    frame_of_mask = np.asarray(sw.run.mask_col)[ex["obj_masks"]]
    pos, frame = R.top_requests(ex["obj_mask_off"], ex["obj_mask_cov"], frame_of_mask, top_k)
    assert (pos[:, 0] >= 0).all() and (top_k < 16 or (pos == -1).any())                    # requests and padding both occur
    np.testing.assert_array_equal(out["top_pos"], pos)
    np.testing.assert_array_equal(out["top_frame"], frame)
    m = min(top_k, 5)
    np.testing.assert_array_equal(out["top_pos"][:, :m], ex["obj_repre"][:, :m])           # the rule of obj_repre
    real = frame >= 0
    ro = np.nonzero(real)[0].astype(np.int32)
    scene = np.asarray(fr.scene_points, np.float32).astype(np.float64)                      # float32 widened exactly
    box, st, ins = ctx.proj_boxes(scene, ex["obj_pt_off"], ex["obj_pts"], k, w2c, W, H, ro, frame[real])
    assert (st == R.OK).sum() >= nf                                                         # the objects are seen in their frames
    for got, want in zip(ctx.proj_boxes(None, ex["obj_pt_off"], ex["obj_pts"], k, w2c, W, H, ro, frame[real],
                                        num_points=len(scene)), (box, st, ins)):            # NULL points: the scene's, widened
        np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(out["boxes"][real], box)
    np.testing.assert_array_equal(out["status"][real], st)
    np.testing.assert_array_equal(out["inside"][real], ins)
    for name in ("boxes", "status", "inside"):
        assert (out[name][~real] == -1).all(), name
    wbox, wst, wins, _ = R.boxes(scene, ex["obj_pt_off"], ex["obj_pts"], k, w2c, W, H, ro, frame[real])
    np.testing.assert_array_equal(box, wbox)
    np.testing.assert_array_equal(st, wst)
    np.testing.assert_array_equal(ins, wins)


def test_sweep_top_views_agrees_with_the_context():
    sw, fr, W, H = _tiny()
    k = np.asarray(fr.intrinsics, np.float64).reshape(-1, 4)
    w2c = np.linalg.inv(np.asarray(fr.poses, np.float64).reshape(-1, 4, 4))
    want = sw.ctx.proj_top_views(k, w2c, W, H, top_k=9)
    for device in (False, True):
        got = sw.top_views(_dev(fr.intrinsics, "float64"), _dev(fr.poses.reshape(-1, 16), "float64"), W, H, device=device)
        assert set(got) == {"top_pos", "top_frame", "boxes", "status", "inside"}
        for name in want:
            np.testing.assert_array_equal(_np(got[name]), want[name], err_msg=name)
    assert want["boxes"].shape == (sw.ctx.pp_info().num_final, 9, 4)


def _raw_boxes(ctx, device, P, points, off, ids, F, k, w2c, W, H, ro, rf):
    """mc_proj_boxes itself on outputs filled with 77: (return code, outputs as numpy)"""
    from maskclustering_amd._native import _ptr
    n = len(ro)
    arrs = [np.ascontiguousarray(points, np.float64), np.ascontiguousarray(off, np.int64), np.ascontiguousarray(ids, np.int32),
            np.ascontiguousarray(k, np.float64), np.ascontiguousarray(w2c, np.float64), np.ascontiguousarray(ro, np.int32),
            np.ascontiguousarray(rf, np.int32)]
    outs = [np.full((n, 4), 77, np.int32), np.full(n, 77, np.int32), np.full(n, 77, np.int32)]
    if device:
        import torch
        arrs = [torch.from_numpy(a).cuda() for a in arrs]
        outs = [torch.from_numpy(a).cuda() for a in outs]
        torch.cuda.synchronize()
        p = [ctypes.c_void_p(a.data_ptr()) for a in arrs + outs]
    else:
        p = [_ptr(a) for a in arrs + outs]
    rc = ctx.L.mc_proj_boxes(ctx.h, P, p[0], len(off) - 1, p[1], p[2], F, p[3], p[4], W, H, n, p[5], p[6], 1 if device else 0,
                             p[7], p[8], p[9], 1 if device else 0)
    ctx.synchronize()
    return rc, [_np(o) for o in outs]


@pytest.mark.parametrize("device", [False, True])
def test_invalid_arguments_leave_the_outputs_untouched(device):
    from maskclustering_amd import _native
    ctx = _ctx()
    rng = np.random.default_rng(0)
    base = dict(P=10, points=rng.normal(0, 1, (10, 3)) + (0, 0, 4), off=[0, 4, 10], ids=list(range(10)), F=2,
                k=[[50.0, 50.0, 32.0, 24.0]] * 2, w2c=np.stack([np.eye(4)] * 2), W=64, H=48, ro=[0, 1, 1], rf=[0, 1, 0])
    rc, outs = _raw_boxes(ctx, device, **base)
    assert rc == _native.MC_OK and (outs[1] == R.OK).all() and (outs[0] != 77).all()       # the base case is valid
    bad = dict(object_index=dict(ro=[0, 2, 1]), negative_object=dict(ro=[-1, 1, 1]), frame_index=dict(rf=[0, 2, 0]),
               point_id=dict(ids=[0, 1, 2, 3, 4, 5, 6, 7, 8, 10]), negative_point_id=dict(ids=[-1] + list(range(1, 10))),
               descending_offset=dict(off=[0, 6, 4]), offset_not_from_zero=dict(off=[1, 4, 10]), width_zero=dict(W=0),
               height_too_large=dict(H=2 ** 30 + 1))
    for name, change in bad.items():
        rc, outs = _raw_boxes(ctx, device, **{**base, **change})
        assert rc == _native.MC_ERR_INVALID, name
        assert all((o == 77).all() for o in outs), name
        assert ctx.L.mc_ctx_last_error(ctx.h)


def test_top_views_states_and_errors():
    from maskclustering_amd import _native
    k, w2c = np.array([[50.0, 50.0, 32.0, 24.0]]), np.eye(4)[None]
    fresh = _native.Context(0)
    with pytest.raises(_native.McError) as e:
        fresh.proj_top_views(k, w2c, 64, 48)                               # before post-processing
    assert e.value.code == _native.MC_ERR_STATE
    sw, fr, W, H = _tiny()
    k = np.asarray(fr.intrinsics, np.float64).reshape(-1, 4)
    w2c = np.linalg.inv(np.asarray(fr.poses, np.float64).reshape(-1, 4, 4))
    for top_k, width in ((17, W), (0, W), (9, 0)):
        n = sw.ctx.pp_info().num_final * 16
        outs = [np.full(n * (4 if i == 2 else 1), 77, np.int32) for i in range(5)]
        rc = sw.ctx.L.mc_proj_top_views(sw.ctx.h, None, len(k), _native._ptr(k), _native._ptr(w2c), width, H, 0, top_k,
                                        *(_native._ptr(o) for o in outs), 0)
        assert rc == _native.MC_ERR_INVALID, (top_k, width)
        assert all((o == 77).all() for o in outs)
    with pytest.raises(_native.McError) as e:
        sw.ctx.proj_top_views(k[:1], w2c[:1], W, H)                        # fewer frames than the scene has
    assert e.value.code == _native.MC_ERR_INVALID


def test_drop_in_returns_the_fixture_tuples_and_nones():
    from maskclustering_amd import top_images
    z = _gold()
    intr = lambda k, W, H: SimpleNamespace(intrinsic_matrix=np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1.0]]),  # noqa: E731
                                           width=W, height=H)
    want = lambda st, box: tuple(int(v) for v in box) if st == R.OK else None  # noqa: E731
    ek = z["edge_intrinsics"]
    for j, name in enumerate(z["edge_name"]):
        pcd = SimpleNamespace(points=z["edge_pts"][j][:z["edge_npts"][j]])
        with np.errstate(all="ignore"):
            got = top_images.get_bbox_by_projection(pcd, intr(ek, *(int(v) for v in z["edge_size"][j])), z["edge_ext"][j])
        assert got == want(z["edge_status"][j], z["edge_box"][j]), name
        assert got is None or all(type(v) is int for v in got)
    _, _, _, fragile = _scene_want()
    for s in range(2):
        W, H = (int(v) for v in z["sizes"][s])
        for j in range(0, len(z["requests"]), 5):
            o, f = z["requests"][j]
            if fragile[s, j]:
                continue
            pcd = SimpleNamespace(points=z["points"][z["obj_pts"][z["obj_pt_off"][o]:z["obj_pt_off"][o + 1]]])
            got = top_images.get_bbox_by_projection(pcd, intr(z["intrinsics"][s, f], W, H), z["extrinsics"][f])
            assert got == want(z["status"][s, j], z["boxes"][s, j]), (s, j)
