"""mc_labels_paint and maskclustering_amd.mask_labels on the GPU, bit-equal to the numpy restatement of
mask_predict.py:94-113 (tests/label_paint_restatement.py; tests/test_label_paint_cpu.py holds it against
the fixture the reference's own program painted): images, status, kept counts, the id -> instance
table and the areas, at the shapes where packing can go wrong (a single pixel, one word more or less,
an odd plane stride that misaligns every plane after the first, a tail word, many waves per plane), for
both mask dtypes, host and device inputs and outputs, the rank and threshold edges, the batch limits,
the overflow at 256 kept, several rounds under a memory budget, every refusal, and the chain into
mc_frames_decode and mc_backproject without a host copy."""
import ctypes

import numpy as np
import pytest

import label_paint_restatement as R

pytestmark = pytest.mark.gpu

KEYS = ("labels", "status", "num_kept", "label_instance", "instance_area")


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _native
    c = _native.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def paint(ctx, masks, scores, off, threshold=0.5, min_pixels=400, device_in=False, device_out=False):
    """mc_labels_paint through the binding, everything as numpy"""
    import torch
    from maskclustering_amd import _native
    prm = _native.paint_params(score_threshold=threshold, min_pixels=min_pixels)
    if device_in:
        masks, scores = torch.from_numpy(np.ascontiguousarray(masks)).cuda(), torch.from_numpy(np.asarray(scores, np.float32)).cuda()
    out = ctx.labels_paint(masks, scores, off, prm, device=device_out)
    if device_out:
        ctx.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in zip(KEYS, out)}


def assert_same(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def ragged(rng, H, W, counts, dtype=np.uint8, density=None):
    """random masks [sum(counts), H, W] (0 / 1, each instance with its own density; the first and last
    pixels and those around the 16-value and 64-bit borders set in every other instance), scores with a
    tie and a NaN, offsets"""
    n = int(np.sum(counts))
    hw = H * W
    m = np.zeros((n, hw), np.uint8)
    for i in range(n):
        d = density if density is not None else rng.choice([0.02, 0.3, 0.7, 1.0])
        m[i] = rng.random(hw) < d
        edge = [p for p in (0, 15, 16, 63, 64, hw - 1) if p < hw]
        m[i, edge] = i & 1
    s = rng.uniform(0, 1, n).astype(np.float32)
    if n >= 4:
        s[1] = s[3]
        s[2] = np.nan
    return m.reshape(n, H, W).astype(dtype), s, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


# ---- the fixture -----------------------------------------------------------------------------------

@pytest.mark.parametrize("device_in", [False, True])
def test_fixture_through_the_c_abi(ctx, golden, device_in):
    for k, fr in enumerate(golden):
        got = paint(ctx, fr["masks"], fr["scores"], [0, len(fr["scores"])], fr["threshold"], device_in=device_in)
        assert got["labels"][0].tobytes() == fr["image"].tobytes(), k
        assert_same(got, R.paint_frames(fr["masks"], fr["scores"], [0, len(fr["scores"])], fr["threshold"]), k)


def test_fixture_through_mask_labels(ctx, golden):
    import torch
    from maskclustering_amd import mask_labels
    for k, fr in enumerate(golden):
        for dev in (False, True):
            m, s = (torch.from_numpy(fr["masks"]).cuda(), torch.from_numpy(fr["scores"]).cuda()) if dev else (fr["masks"], fr["scores"])
            img = mask_labels.label_image(m, s, confidence_threshold=fr["threshold"], ctx=ctx)
            assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == fr["image"].shape
            assert mask_labels.to_host(img).tobytes() == fr["image"].tobytes(), (k, dev)
    batch = [golden[k] for k in (0, 1, 2, 4)]  # the float32 48 x 40 frames of the run at 0.5
    res = mask_labels.label_images([(torch.from_numpy(f["masks"]).cuda(), torch.from_numpy(f["scores"]).cuda()) for f in batch], ctx=ctx)
    assert tuple(res.labels.shape) == (4, 48, 40) and res.labels.is_cuda
    for k, fr in enumerate(batch):
        assert mask_labels.to_host(res.labels[k]).tobytes() == fr["image"].tobytes()
        kept = R.paint_frame(fr["masks"], fr["scores"])[1]
        assert res.num_kept[k] == len(kept) and list(res.label_instance[k, :len(kept)]) == list(kept)
    assert mask_labels.label_image(golden[0]["masks"], golden[0]["scores"]).cpu().numpy().tobytes() == golden[0]["image"].tobytes()


# ---- shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (1, 63), (1, 64), (1, 65), (23, 37), (16, 16), (64, 64), (48, 40)])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_shapes_where_packing_can_go_wrong(ctx, shape, dtype):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    m, s, off = ragged(rng, H, W, [3, 0, 7, 1, 12, 0], dtype)
    mp = max(1, min(4, H * W // 4))
    want = R.paint_frames(m, s, off, 0.25, mp)
    assert want["num_kept"].max() >= 1
    assert_same(paint(ctx, m, s, off, 0.25, mp), want, "host")
    assert_same(paint(ctx, m, s, off, 0.25, mp, device_in=True, device_out=True), want, "device")
    assert_same(paint(ctx, m, s, off, 0.25, mp, device_in=True), want, "device in, host out")


def test_one_set_pixel_at_every_border_and_no_tail_bit_leaks(ctx):
    for H, W in ((1, 63), (1, 65), (23, 37), (5, 16)):
        hw = H * W
        spots = [p for p in (0, 15, 16, 63, 64, hw - 1) if p < hw]
        m = np.zeros((len(spots) + 1, hw), np.uint8)
        for i, p in enumerate(spots):
            m[i, p] = 1
        m[-1] = 1  # the whole image: its area is hw, not the 64 * words bits of its plane
        s = np.linspace(0.9, 0.3, len(m)).astype(np.float32)
        for arr in (m, m.astype(np.float32)):
            arr = arr.reshape(-1, H, W)
            want = R.paint_frames(arr, s, [0, len(m)], 0.2, 1)
            assert list(want["instance_area"]) == [1] * len(spots) + [hw] and want["num_kept"][0] == len(m)
            assert_same(paint(ctx, arr, s, [0, len(m)], 0.2, 1, device_in=True), want, (H, W))


def test_a_full_image_instance_at_480_x_640_counts_across_many_waves(ctx):
    H, W = 480, 640
    rng = np.random.default_rng(1)
    m = np.zeros((4, H, W), np.uint8)
    m[0] = 1
    m[1, 100:300, 200:500] = 1
    m[2] = rng.random((H, W)) < 0.4
    m[3, -1, -1] = 1
    s = np.array([0.6, 0.9, 0.8, 0.99], np.float32)
    want = R.paint_frames(m, s, [0, 4])
    assert want["instance_area"][0] == 307200 and list(want["label_instance"][0, :4]) == [0, 2, 1, -1]
    assert_same(paint(ctx, m, s, [0, 4], device_in=True, device_out=True), want)
    assert_same(paint(ctx, m.astype(np.float32), s, [0, 4], device_in=True), want)


# ---- mask values -----------------------------------------------------------------------------------

def test_only_the_value_one_is_set_and_both_encodings_agree(ctx):
    rng = np.random.default_rng(2)
    H, W = 23, 37
    u8 = rng.choice(np.array([0, 1, 2, 255], np.uint8), (6, H, W))
    s = rng.uniform(0.3, 1, 6).astype(np.float32)
    want = R.paint_frames(u8, s, [0, 2, 6], 0.25, 4)
    assert list(want["instance_area"]) == list((u8 == 1).sum(axis=(1, 2)))
    assert_same(paint(ctx, u8, s, [0, 2, 6], 0.25, 4, device_in=True), want)
    f32 = rng.choice(np.array([0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 2.0, -1.0, np.nan], np.float32), (6, H, W))
    wantf = R.paint_frames(f32, s, [0, 2, 6], 0.25, 4)
    assert list(wantf["instance_area"]) == list((f32 == 1).sum(axis=(1, 2)))
    assert_same(paint(ctx, f32, s, [0, 2, 6], 0.25, 4, device_in=True), wantf)
    assert_same(paint(ctx, f32, s, [0, 2, 6], 0.25, 4), wantf)
    # the same masks as uint8, bool and float32
    b = u8 == 1
    got = [paint(ctx, a, s, [0, 2, 6], 0.25, 4, device_in=True) for a in (b.astype(np.uint8), b, b.astype(np.float32))]
    assert_same(got[0], want), assert_same(got[1], want), assert_same(got[2], want)


# ---- rank and threshold ----------------------------------------------------------------------------

@pytest.mark.parametrize("threshold", [0.7, 0.1])
def test_scores_around_the_threshold_ties_zeros_and_nan(ctx, threshold):
    f32 = np.float32
    t = f32(threshold)
    rng = np.random.default_rng(3)
    s = np.array([t, np.nextafter(t, f32(0)), np.nextafter(t, f32(1)), 0.9, 0.9, np.nan, 0.9, np.inf, 0.9, t, -np.inf, 0.95],
                 f32)
    m, _, off = ragged(rng, 16, 16, [len(s)], density=0.3)
    want = R.paint_frames(m, s, off, threshold, 4)
    assert list(want["label_instance"][0, :int(want["num_kept"][0])]) == [0, 9, 2, 3, 4, 6, 8, 11, 7]
    assert_same(paint(ctx, m, s, off, threshold, 4, device_in=True), want)
    # -0.0 and +0.0 tie by index (threshold below them), among many equal scores
    z = np.array([0.0, -0.0, 0.0, -0.0, 0.5, 0.5, 0.5, -0.0, 0.0, 0.5], f32)
    m, _, off = ragged(rng, 16, 16, [len(z)], density=0.3)
    want = R.paint_frames(m, z, off, -1.0, 4)
    assert list(want["label_instance"][0, :10]) == [0, 1, 2, 3, 7, 8, 4, 5, 6, 9]
    assert_same(paint(ctx, m, z, off, -1.0, 4, device_in=True), want)


# ---- batches ---------------------------------------------------------------------------------------

def test_empty_frames_single_instances_and_1024_instances(ctx):
    rng = np.random.default_rng(4)
    m, s, off = ragged(rng, 8, 8, [0, 0, 5, 0, 1, 1024, 1, 0])
    s[:] = rng.uniform(0, 1, len(s)).astype(np.float32)
    s[6 + 100] = s[6 + 900]  # a tie far apart
    want = R.paint_frames(m, s, off, 0.9, 4)
    assert 1 <= want["num_kept"][5] <= 255 and not want["labels"][[0, 1, 3, 7]].any()
    assert_same(paint(ctx, m, s, off, 0.9, 4), want, "host")
    assert_same(paint(ctx, m, s, off, 0.9, 4, device_in=True, device_out=True), want, "device")
    none = paint(ctx, np.zeros((0, 8, 8), np.uint8), np.zeros(0, np.float32), [0, 0, 0])
    assert_same(none, R.paint_frames(np.zeros((0, 8, 8), np.uint8), np.zeros(0, np.float32), [0, 0, 0]))


def raw_call(ctx, F, H, W, off, dtype, n, prm=None):
    """mc_labels_paint on sentinel-filled device arrays; (return code, arrays after the call)"""
    import torch
    from maskclustering_amd import _native
    prm = prm or _native.paint_params()
    off = np.ascontiguousarray(off, np.int64)
    hw = H * W if 0 < H * W <= 1 << 20 else 1  # a refused size is never read or written
    masks = torch.ones(max(n, 1) * hw, dtype=torch.uint8, device="cuda")
    scores = torch.full((max(n, 1),), 0.9, dtype=torch.float32, device="cuda")
    labels = torch.full((max(F, 1) * hw,), 77, dtype=torch.uint8, device="cuda")
    small = [torch.full((k,), -7, dtype=torch.int32, device="cuda") for k in (max(F, 1), max(F, 1), max(F, 1) * 255, max(n, 1))]
    torch.cuda.synchronize()
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = ctx.L.mc_labels_paint(ctx.h, F, H, W, off.ctypes.data_as(ctypes.c_void_p), dtype, p(masks), p(scores), 1,
                               ctypes.byref(prm), p(labels), *[p(t) for t in small], 1)
    ctx.synchronize()
    return rc, ctx.L.mc_ctx_last_error(ctx.h).decode(), [labels.cpu().numpy()] + [t.cpu().numpy() for t in small]


def untouched(arrays):
    return (arrays[0] == 77).all() and all((a == -7).all() for a in arrays[1:])


def test_1025_instances_are_refused_with_nothing_written(ctx):
    from maskclustering_amd import _native
    rc, msg, arrays = raw_call(ctx, 2, 8, 8, [0, 3, 3 + 1025], _native.MC_PAINT_U8, 3 + 1025)
    assert rc == _native.MC_ERR_INVALID and "frame 1" in msg and "1024" in msg and untouched(arrays)
    rc, msg, arrays = raw_call(ctx, 2, 8, 8, [0, 3, 3 + 1024], _native.MC_PAINT_U8, 3 + 1024)
    assert rc == _native.MC_OK and not untouched(arrays)


def test_every_invalid_argument_is_refused_before_a_launch(ctx):
    from maskclustering_amd import _native
    u8 = _native.MC_PAINT_U8
    cases = [
        (dict(F=2, H=8, W=8, off=[0, 5, 4], dtype=u8, n=5), "non-decreasing"),
        (dict(F=2, H=8, W=8, off=[1, 2, 3], dtype=u8, n=3), "inst_off[0]"),
        (dict(F=1, H=8, W=8, off=[0, 1025], dtype=u8, n=1025), "MC_PAINT_MAX_INSTANCES"),
        (dict(F=1, H=8, W=8, off=[0, 2], dtype=2, n=2), "mask_dtype"),
        (dict(F=1, H=8, W=8, off=[0, 2], dtype=-1, n=2), "mask_dtype"),
        (dict(F=1, H=0, W=8, off=[0, 2], dtype=u8, n=2), "H or W"),
        (dict(F=1, H=8, W=-3, off=[0, 2], dtype=u8, n=2), "H or W"),
        (dict(F=1, H=46341, W=46341, off=[0, 0], dtype=u8, n=0), "2^31"),
        (dict(F=1, H=8, W=8, off=[0, 2], dtype=u8, n=2, prm=_native.paint_params(min_pixels=-1)), "min_pixels"),
    ]
    for kw, word in cases:
        rc, msg, arrays = raw_call(ctx, **kw)
        assert rc == _native.MC_ERR_INVALID and word in msg and untouched(arrays), (kw, msg)
    with pytest.raises(_native.McError) as e:
        paint(ctx, np.ones((2, 4, 4), np.uint8), [0.9, 0.8], [0, 2], min_pixels=-5)
    assert e.value.code == _native.MC_ERR_INVALID
    # the context still works
    rc, _, arrays = raw_call(ctx, 1, 8, 8, [0, 2], u8, 2, prm=_native.paint_params(min_pixels=4))
    assert rc == _native.MC_OK and (arrays[0][:64] == 2).all() and arrays[2][0] == 2


# ---- overflow --------------------------------------------------------------------------------------

def test_255_kept_paint_every_id_and_the_256th_overflows_its_frame_only(ctx):
    import torch
    from maskclustering_amd import _native, mask_labels
    H, W = 16, 16
    rng = np.random.default_rng(6)
    m = np.zeros((255 + 3 + 256 + 2, H * W), np.uint8)
    for i in range(len(m)):
        m[i, i % 256] = 1                    # its own pixel: with 255 kept every id owns one
        if i >= 255:
            m[i, rng.integers(0, 256, 3)] = 1
    m = m.reshape(-1, H, W)
    s = rng.uniform(0.5, 1, len(m)).astype(np.float32)
    off = [0, 255, 258, 258 + 256, len(m)]
    want = R.paint_frames(m, s, off, 0.5, 1)
    assert list(want["status"]) == [0, 0, 1, 0] and list(want["num_kept"]) == [255, 3, 256, 2]
    assert set(np.unique(want["labels"][0])) == set(range(1, 256)) | {0} and not want["labels"][2].any()
    assert_same(paint(ctx, m, s, off, 0.5, 1, device_in=True), want)
    assert_same(paint(ctx, m, s, off, 0.5, 1, device_out=True), want)
    frames = [(torch.from_numpy(m[a:b]).cuda(), torch.from_numpy(s[a:b]).cuda()) for a, b in zip(off[:-1], off[1:])]
    with pytest.raises(OverflowError, match="frame 2"):
        mask_labels.label_images(frames, min_pixels=1, ctx=ctx)
    with pytest.raises(OverflowError):
        mask_labels.label_image(*frames[2], min_pixels=1, ctx=ctx)
    assert mask_labels.label_images(frames[:2], min_pixels=1, ctx=ctx).labels.cpu().numpy().tobytes() == want["labels"][:2].tobytes()
    assert _native.MC_PAINT_OVERFLOW == 1


# ---- budget, determinism ---------------------------------------------------------------------------

def test_a_budget_that_forces_rounds_gives_the_same_bits_and_one_below_a_frame_is_refused(ctx):
    from maskclustering_amd import _native
    rng = np.random.default_rng(7)
    H, W = 23, 37
    m, s, off = ragged(rng, H, W, [4, 0, 9, 2, 0, 6, 1], np.float32)
    want = R.paint_frames(m, s, off, 0.25, 40)
    words = (H * W + 63) // 64
    try:
        for staged, per in ((False, words * 8), (True, words * 8 + 4 * H * W)):
            for n in (9, 10, 13, 22):  # 9: the largest frame alone; more: two or three frames a round
                ctx.set_memory_budget(n * per)
                assert_same(paint(ctx, m, s, off, 0.25, 40, device_in=not staged), want, (staged, n))
            ctx.set_memory_budget(9 * per - 1)
            with pytest.raises(_native.McError) as e:
                paint(ctx, m, s, off, 0.25, 40, device_in=not staged)
            assert e.value.code == _native.MC_ERR_UNSUPPORTED and "frame 2" in str(e.value)
    finally:
        ctx.set_memory_budget(0)
    assert_same(paint(ctx, m, s, off, 0.25, 40), want, "no budget")


def test_two_runs_are_bit_equal(ctx):
    rng = np.random.default_rng(8)
    m, s, off = ragged(rng, 64, 64, [30, 0, 50, 20])
    a = paint(ctx, m, s, off, 0.3, 100, device_in=True, device_out=True)
    b = paint(ctx, m, s, off, 0.3, 100, device_in=True, device_out=True)
    assert_same(a, b)
    assert_same(a, R.paint_frames(m, s, off, 0.3, 100))


# ---- the chain -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene_masks():
    """eight 48 x 40 frames of the tiny synthetic scene, with five objects large and dense enough that
    S1 keeps three or four masks a frame at this resolution (the CPU oracle's count); per frame the
    instance masks of its segmentation with random scores (frame 3 without instances)"""
    from maskclustering_amd.synthetic_frames import make_frames_shape
    sc = make_frames_shape("tiny", seed=5, H=48, W=40, size=(0.5, 1.0), num_objects=5, spacing=0.01)
    rng = np.random.default_rng(9)
    frames = []
    for f in range(sc.num_frames):
        ids = [i for i in np.unique(sc.seg[f]) if i] if f != 3 else []
        m = np.stack([sc.seg[f] == i for i in ids]).astype(np.float32) if ids else np.zeros((0, 48, 40), np.float32)
        frames.append((m, rng.uniform(0.4, 1, len(ids)).astype(np.float32)))
    assert sc.num_frames == 8 and sum(len(s) for _, s in frames) >= 8
    return sc, frames


def test_painted_labels_resized_by_frames_decode_on_the_device(ctx, scene_masks):
    import torch
    from maskclustering_amd import mask_labels
    from oracle import io_oracle
    sc, frames = scene_masks
    big = [(np.repeat(np.repeat(m, 2, axis=1), 2, axis=2), s) for m, s in frames]  # the model's 96 x 80
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in big])])
    want = R.paint_frames(np.concatenate([m for m, _ in big]), np.concatenate([s for _, s in big]), off, 0.5, 16)
    assert want["labels"].any() and want["labels"].shape == (8, 96, 80)
    res = mask_labels.label_images([(torch.from_numpy(m).cuda(), torch.from_numpy(s).cuda()) for m, s in big], min_pixels=16, ctx=ctx)
    assert res.labels.cpu().numpy().tobytes() == want["labels"].tobytes()
    small = torch.empty((8, 48, 40), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.frames_decode(8, 48, 40, None, 1000.0, (96, 80), res.labels.data_ptr(), True, None, small.data_ptr())
    assert small.cpu().numpy().tobytes() == io_oracle.resize_nearest(want["labels"], 48, 40).tobytes()


def test_backproject_fed_the_device_labels_equals_backproject_fed_the_host_image(ctx, scene_masks):
    import torch
    from maskclustering_amd import mask_labels
    sc, frames = scene_masks
    off = np.concatenate([[0], np.cumsum([len(s) for _, s in frames])])
    want = R.paint_frames(np.concatenate([m for m, _ in frames]), np.concatenate([s for _, s in frames]), off, 0.5, 16)
    res = mask_labels.label_images([(torch.from_numpy(m).cuda(), torch.from_numpy(s).cuda()) for m, s in frames], min_pixels=16, ctx=ctx)
    ctx.set_points(np.asarray(sc.scene_points, np.float64).astype(np.float32))
    ctx.backproject(sc.depth, want["labels"], sc.intrinsics, sc.poses)
    host = ctx.bp_masks()
    assert len(host[0]) >= 4
    dev = [torch.from_numpy(np.ascontiguousarray(a, dt)).cuda() for a, dt in
           ((sc.depth, np.float32), (sc.intrinsics, np.float64), (np.asarray(sc.poses).reshape(8, 16), np.float64))]
    torch.cuda.synchronize()
    ctx.backproject(None, None, None, None, device_ptrs=(dev[0].data_ptr(), res.labels.data_ptr(), dev[1].data_ptr(), dev[2].data_ptr()),
                    shape=(8, 48, 40))
    got = ctx.bp_masks()
    for a, b in zip(got, host):
        assert a.tobytes() == b.tobytes()
