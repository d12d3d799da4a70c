"""Scene point cloud fusion on the device (mc_cloud_*, maskclustering_amd/scene_cloud.py) against the numpy
restatement (tests/scene_cloud_restatement.py): every result BIT-EQUAL, points, colours and order; no
tolerance anywhere.  The shapes are tiny (7 frames of 48 x 64); the voxel size alone moves the largest
voxel population through every class of the ordered fold (a thread, a workgroup in LDS, a workgroup in
global memory), whose thresholds are read out of csrc/mc_cloud_plan.hpp."""
import os
import re

import numpy as np
import pytest

import scene_cloud_restatement as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def constants():
    src = open(os.path.join(REPO, "maskclustering_amd", "csrc", "mc_cloud_plan.hpp")).read()
    out = {}
    for name in ("kCloudThreadMax", "kCloudLdsMax"):
        m = re.findall(r"constexpr int %s = (\d+);" % name, src)
        assert len(m) == 1, name
        out[name] = int(m[0])
    return out


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@pytest.fixture(scope="module")
def frames():
    """7 frames of 48 x 64, frame 4 with a pose whose row 3 is not (0, 0, 0, 1); read-only"""
    fr = R.synthetic_frames(7, 48, 64, seed=0, general_pose_frame=4)
    assert np.array_equal(fr[3][0, 3], [0, 0, 0, 1]) and not np.array_equal(fr[3][4, 3], [0, 0, 0, 1])
    for a in fr:
        a.setflags(write=False)
    return fr


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def fuse(ctx, depth, rgb, K, T, voxel, B, trunc=20.0):
    from maskclustering_amd.scene_cloud import fuse_frames
    p, c = fuse_frames(depth, rgb, K, T, voxel_size=voxel, buffer_size=B, depth_trunc=trunc, ctx=ctx)
    return p, c, ctx.cloud_info()


def check(ctx, depth, rgb, K, T, voxel, B):
    """the device result against the restatement; returns (cloud_info, the restatement's populations)"""
    info = {}
    wp, wc = R.fuse_frames(depth, rgb, K, T, voxel, B, info=info)
    p, c, ci = fuse(ctx, depth, rgb, K, T, voxel, B)
    assert same(p, wp), "points"
    assert same(c, wc), "colours"
    pops = info["populations"]
    assert ci["num_points"] == len(wp) and ci["max_stage_points"] == max(info["sizes"])
    assert ci["max_voxel_population"] == max([int(x.max()) for x in pops if len(x)] + [0])
    return ci, pops


def test_golden_of_the_reference_function(ctx):
    from test_scene_cloud_cpu import golden_frames
    g, depth, rgb, K, T = golden_frames()
    p, c, _ = fuse(ctx, depth, rgb, K, T, float(g["voxel_size"]), int(g["buffer_size"]))
    assert same(p, g["points"]) and same(c, g["colors"])


@pytest.mark.parametrize("voxel", [0.005, 0.05, 0.5, 5.0])
def test_voxel_sizes_move_the_population_through_every_fold_class(ctx, frames, voxel):
    k = constants()
    ci, pops = check(ctx, *frames, voxel, 3)
    assert ci["stages"] == 4
    big = ci["max_voxel_population"]
    if voxel == 0.005:
        assert big <= k["kCloudThreadMax"]
    if voxel == 0.5:
        assert any(((x > k["kCloudThreadMax"]) & (x <= k["kCloudLdsMax"])).any() for x in pops)
    if voxel == 5.0:
        assert big > k["kCloudLdsMax"]


@pytest.mark.parametrize("which", ["kCloudThreadMax", "kCloudLdsMax"])
def test_a_voxel_of_exactly_the_threshold_population_and_of_one_more(ctx, frames, which):
    """One voxel holds a whole buffer (voxel size 50 m); the first buffer keeps exactly the threshold's
    number of valid pixels, the second one more."""
    t = constants()[which]
    depth, rgb, K, T = frames
    d = depth.copy()
    for f0, keep in ((0, t), (3, t + 1)):
        buf = d[f0:f0 + 3].reshape(-1)
        valid = np.nonzero(R.valid_pixels(buf))[0]
        assert len(valid) > keep
        buf[valid[np.linspace(0, len(valid) - 1, len(valid) - keep).round().astype(int)]] = 0.0  # spread over the frames
    _, pops = check(ctx, d, rgb, K, T, 50.0, 3)
    assert pops[0].tolist() == [t] and pops[1].tolist() == [t + 1]


@pytest.mark.parametrize("F,B", [(6, 3), (2, 3), (3, 1)])
def test_schedules(ctx, frames, F, B):
    ci, _ = check(ctx, *(a[:F] for a in frames), 0.05, B)
    assert ci["stages"] == len(R.flush_schedule(F, B)) + 1


def test_a_full_buffer_without_a_valid_pixel_and_an_empty_result(ctx, frames):
    depth, rgb, K, T = frames
    d = depth.copy()
    d[:3] = 0.0
    ci, _ = check(ctx, d, rgb, K, T, 0.05, 3)
    assert ci["num_points"] > 0
    d[:] = np.nan
    ci, _ = check(ctx, d, rgb, K, T, 0.05, 3)
    assert ci["num_points"] == 0
    p, c = ctx.cloud_get()
    assert p.shape == (0, 3) and c.shape == (0, 3)
    ci, _ = check(ctx, d[:0], rgb[:0], K[:0], T[:0], 0.05, 3)  # F = 0
    assert ci["num_points"] == 0


def test_a_voxel_first_seen_in_a_later_frame_keeps_its_place_in_the_order(ctx, frames):
    depth, rgb, K, T = frames
    d = np.stack([depth[0], depth[0]])
    d[0, :, 1::2] = 0.0  # frame 0 sees the even columns, frame 1 the odd ones, from the same camera
    d[1, :, 0::2] = 0.0
    two = (d, rgb[:2], np.stack([K[0], K[0]]), np.stack([T[0], T[0]]))
    check(ctx, *two, 0.02, 2)
    wp, _ = R.fuse_frames(*two, 0.02, 2)
    lone, _ = R.fuse_frames(d[:1], rgb[:1], K[:1], T[:1], 0.02, 2)
    assert len(wp) > len(lone)  # frame 1 opened voxels of its own, listed after frame 0's


def test_depth_edges(ctx, frames):
    depth, rgb, K, T = frames
    d = np.full((1, 48, 64), 0.0, np.float32)
    edge = [0.0, -1.0, np.nan, np.inf, 20.0, np.nextafter(np.float32(20.0), np.float32(0.0)), 1.0]
    d[0, 5, :7] = edge
    ci, _ = check(ctx, d, rgb[:1], K[:1], T[:1], 0.005, 3)
    assert ci["num_points"] == 2  # the last two are kept


def test_device_tensors_in_and_out(ctx, frames):
    import torch
    from maskclustering_amd.scene_cloud import fuse_frames
    wp, wc = R.fuse_frames(*frames, 0.05, 3)
    dev = [torch.from_numpy(np.array(a)).to("cuda:0") for a in frames]  # (writable copies of the read-only frames)
    p, c = fuse_frames(*dev, voxel_size=0.05, buffer_size=3, ctx=ctx)
    torch.cuda.synchronize()
    assert p.is_cuda and same(p.cpu().numpy(), wp) and same(c.cpu().numpy(), wc)


def test_voxel_down_on_arrays(ctx, frames):
    depth, rgb, K, T = frames
    fp = [R.frame_points(depth[f], rgb[f], K[f], T[f]) for f in range(3)]
    p, c = np.concatenate([a for a, _ in fp]), np.concatenate([b for _, b in fp])
    for voxel in (0.05, 0.5):
        wp, wc, cnt = R.voxel_down_sample(p, c, voxel)
        ci = ctx.cloud_voxel_down(p, c, voxel)
        gp, gc = ctx.cloud_get()
        assert same(gp, wp) and same(gc, wc)
        assert ci["stages"] == 1 and ci["max_stage_points"] == len(p) and ci["max_voxel_population"] == int(cnt.max())
        # a one-buffer run of the frame route is this stage and the final pass over its result
        ctx.cloud_voxel_down(gp, gc, voxel)
        twice = ctx.cloud_get()
        fr = fuse(ctx, depth[:3], rgb[:3], K[:3], T[:3], voxel, 3)
        assert same(twice[0], fr[0]) and same(twice[1], fr[1])
    # no colours
    wp, _, _ = R.voxel_down_sample(p, None, 0.05)
    ctx.cloud_voxel_down(p, None, 0.05)
    gp, gc = ctx.cloud_get(colors=False)
    assert same(gp, wp) and gc is None
    from maskclustering_amd._native import McError, MC_ERR_STATE
    with pytest.raises(McError) as e:
        ctx.cloud_get()
    assert e.value.code == MC_ERR_STATE
    # far from the origin, negative coordinates
    far = p * np.array([1.0, -1.0, 1.0]) - 1e4
    wp, wc, _ = R.voxel_down_sample(far, c, 0.005)
    ctx.cloud_voxel_down(far, c, 0.005)
    gp, gc = ctx.cloud_get()
    assert same(gp, wp) and same(gc, wc) and (gp < 0).all()


def test_extent_of_two_to_the_21_voxels(ctx):
    from maskclustering_amd._native import McError, MC_ERR_UNSUPPORTED
    vs = 0.5
    ok = np.array([[0.0, 0.0, 0.0], [0.0, (2 ** 21 - 1) * vs, 0.0]])
    wp, _, _ = R.voxel_down_sample(ok, None, vs)
    ctx.cloud_voxel_down(ok, None, vs)
    assert same(ctx.cloud_get(colors=False)[0], wp) and len(wp) == 2
    over = np.array([[0.0, 0.0, 0.0], [0.0, 2 ** 21 * vs, 0.0]])
    with pytest.raises(McError) as e:
        ctx.cloud_voxel_down(over, None, vs)
    assert e.value.code == MC_ERR_UNSUPPORTED and "2^21" in str(e.value)
    assert same(ctx.cloud_get(colors=False)[0], wp)  # the earlier result stands


def test_refusals_leave_the_earlier_result(ctx, frames):
    from maskclustering_amd._native import McError, MC_ERR_INVALID, MC_ERR_UNSUPPORTED
    depth, rgb, K, T = frames
    wp, wc, _ = fuse(ctx, depth, rgb, K, T, 0.05, 3)
    before = ctx.cloud_info()

    def unchanged():
        p, c = ctx.cloud_get()
        return same(p, wp) and same(c, wc) and ctx.cloud_info() == before

    bad_T = T.copy()
    bad_T[2, 1, 3] = np.inf
    bad_K = K.copy()
    bad_K[6, 0] = np.nan
    for args, code in (((depth, rgb, K, bad_T, 0.05, 3), MC_ERR_INVALID), ((depth, rgb, bad_K, T, 0.05, 3), MC_ERR_INVALID),
                       ((depth, rgb, K, T, 0.0, 3), MC_ERR_INVALID), ((depth, rgb, K, T, -1.0, 3), MC_ERR_INVALID),
                       ((depth, rgb, K, T, 0.05, 0), MC_ERR_INVALID)):
        with pytest.raises(McError) as e:
            fuse(ctx, *args)
        assert e.value.code == code and unchanged()
    pts = np.array([[0.0, 0.0, 0.0], [1.0, np.nan, 0.0]])
    with pytest.raises(McError) as e:
        ctx.cloud_voxel_down(pts, None, 0.05)
    assert e.value.code == MC_ERR_INVALID and unchanged()
    ctx.set_memory_budget(100000)  # the stages here need several hundred kilobytes
    try:
        with pytest.raises(McError) as e:
            fuse(ctx, depth, rgb, K, T, 0.05, 3)
        assert e.value.code == MC_ERR_UNSUPPORTED and re.search(r"needs? \d+ bytes", str(e.value)) and unchanged()
    finally:
        ctx.set_memory_budget(0)
    p, c, _ = fuse(ctx, depth, rgb, K, T, 0.05, 3)
    assert same(p, wp) and same(c, wc)


def test_getters_before_a_result():
    from maskclustering_amd import _native
    c = _native.Context(0)
    try:
        for call in (c.cloud_info, c.cloud_get, c.scene_use_cloud):
            with pytest.raises(_native.McError) as e:
                call()
            assert e.value.code == _native.MC_ERR_STATE
    finally:
        c.close()


def test_the_same_call_twice_and_in_a_fresh_context_gives_the_same_bytes(ctx, frames):
    from maskclustering_amd import _native
    a = fuse(ctx, *frames, 0.5, 3)
    b = fuse(ctx, *frames, 0.5, 3)
    other = _native.Context(0)
    try:
        c = fuse(other, *frames, 0.5, 3)
    finally:
        other.close()
    for x in (b, c):
        assert same(a[0], x[0]) and same(a[1], x[1]) and a[2] == x[2]


def test_scene_use_cloud_equals_set_points_of_the_rounded_points(ctx):
    from maskclustering_amd import _native
    from maskclustering_amd.synthetic_frames import make_frames_shape
    fr = make_frames_shape("tiny", seed=0)
    ctx.cloud_voxel_down(np.ascontiguousarray(fr.scene_points, np.float64), None, 0.01)
    pts, _ = ctx.cloud_get(colors=False)
    assert len(pts) > 100
    ctx.scene_use_cloud()
    ctx.backproject(fr.depth, fr.seg, fr.intrinsics, fr.poses)
    got = ctx.bp_masks()
    other = _native.Context(0)
    try:
        other.set_points(pts.astype(np.float32))
        other.backproject(fr.depth, fr.seg, fr.intrinsics, fr.poses)
        want = other.bp_masks()
    finally:
        other.close()
    assert len(want[0]) > 0
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


def test_create_downsampled_point_cloud_reads_a_scene_directory(ctx, frames, tmp_path):
    from PIL import Image
    from maskclustering_amd.scene_cloud import create_downsampled_point_cloud
    depth, rgb, K, T = (a[:5] for a in frames)
    for sub in ("depth", "color", "pose", "intrinsic"):
        os.makedirs(tmp_path / sub)
    m = np.eye(4)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = K[0]
    np.savetxt(tmp_path / "intrinsic" / "intrinsic_depth.txt", m)
    ids = ["10", "2", "33", "4", "21"]  # string order and integer order differ
    d16 = np.round(depth.astype(np.float64) * 1000).astype(np.uint16)
    for k, fid in enumerate(ids):
        Image.fromarray(d16[k]).save(tmp_path / "depth" / f"{fid}.png")
        Image.fromarray(rgb[k]).save(tmp_path / "color" / f"{fid}.jpg", format="PNG")  # lossless under the .jpg name
        np.savetxt(tmp_path / "pose" / f"{fid}.txt", T[k])
    order = [1, 0, 2]  # 2, 4, 10, 21, 33 by integer value; every second: 2, 10, 33
    dd = (d16[order].astype(np.float64) / 1000).astype(np.float32)
    wp, wc = R.fuse_frames(dd, rgb[order], np.tile(K[0], (3, 1)), T[order], 0.05, 2)
    p, c = create_downsampled_point_cloud(str(tmp_path), image_size=(64, 48), stride=2, depth_trunc=0.05, buffer_size=2,
                                          depth_scale=1000, ctx=ctx)
    assert same(p, wp) and same(c, wc)
    Image.fromarray(rgb[0][:10]).save(tmp_path / "color" / "4.jpg", format="PNG")
    with pytest.raises(ValueError, match="resize"):
        create_downsampled_point_cloud(str(tmp_path), ctx=ctx)
