"""Device CLIP crop preparation (mc_crop_boxes / mc_crop_render / mc_crop_coeffs and
maskclustering_amd.semantics.get_open_voc_features) against the fixtures made by the reference's
own code (tests/golden/make_clip_crops_golden.py) and the numpy restatement
(tests/clip_crops_restatement.py).  Everything is bit-equal except the features, whose bound is
derived in test_extract_features_equals_reference_main.  Neither Pillow nor the reference is needed."""
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest

import clip_crops_model
import clip_crops_restatement as R
from conftest import GOLDEN, REPO

pytestmark = pytest.mark.gpu

SIDES = list(range(1, 65)) + [113, 223, 224, 225, 447, 448, 449, 777, 1000, 1440, 1920]


def _gold(name):
    z = dict(np.load(os.path.join(GOLDEN, name)))
    if "requests" in z:
        z["req"] = [tuple(int(v) for v in r) for r in z["requests"]]
    return z


@pytest.fixture(scope="module")
def ctx():
    from maskclustering_amd import _device
    return _device.context()


@pytest.fixture(scope="module")
def golds():
    out = {}
    for name in ("clip_crops_small.npz", "clip_crops_224.npz"):
        z = _gold(name)
        z["boxes"], st = R.boxes_and_status(z["seg"], z["req"])
        assert np.array_equal(st, z["status"])
        z["want"] = R.to_float(z["pixels"], z["status"], z["tables"])
        out[name] = z
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(z):
    from maskclustering_amd import _native
    return _native.crop_params(out_size=int(z["out_size"]))


def _render(ctx, z, chunk, device_boxes, prm=None):
    import torch
    prm = prm or _params(z)
    mf = np.array([f for f, _ in z["req"]], np.int32)
    ml = np.array([m for _, m in z["req"]], np.int32)
    rgb = torch.as_tensor(z["rgb"]).cuda() if device_boxes else z["rgb"]
    seg = torch.as_tensor(z["seg"]).cuda() if device_boxes else z["seg"]
    boxes, status = ctx.crop_boxes(seg, mf, ml, prm, device=device_boxes)
    parts = [ctx.crop_render(rgb, mf[i:i + chunk], boxes[i:i + chunk], status[i:i + chunk], prm)
             for i in range(0, len(mf), chunk)]
    return torch.cat(parts).cpu().numpy()


@pytest.mark.parametrize("name", ["clip_crops_small.npz", "clip_crops_224.npz"])
def test_boxes_and_status_equal_fixture_host_and_device(ctx, golds, name):
    import torch
    z = golds[name]
    mf = np.array([f for f, _ in z["req"]], np.int32)
    ml = np.array([m for _, m in z["req"]], np.int32)
    for seg in (z["seg"], torch.as_tensor(z["seg"]).cuda()):
        for device in (False, True):
            boxes, status = ctx.crop_boxes(seg, mf, ml, _params(z), device=device)
            if device:
                boxes, status = boxes.cpu().numpy(), status.cpu().numpy()
            np.testing.assert_array_equal(status, z["status"])
            np.testing.assert_array_equal(boxes, z["boxes"])


@pytest.mark.parametrize("chunk,device_boxes", [(1 << 20, False), (1, False), (5, False), (5, True), (1 << 20, True)])
@pytest.mark.parametrize("name", ["clip_crops_small.npz", "clip_crops_224.npz"])
def test_render_equals_fixture_bit_for_bit(ctx, golds, name, chunk, device_boxes):
    z = golds[name]
    got = _render(ctx, z, chunk, device_boxes)
    assert got.shape == z["want"].shape
    np.testing.assert_array_equal(_bits(got), _bits(z["want"]))


@pytest.mark.parametrize("out_size", [224, 32])
def test_device_coefficient_tables_equal_restatement(ctx, out_size):
    for s in SIDES:
        ksize, bounds, kk = R.coeffs(s, out_size)
        k, b, t = ctx.crop_coeffs(s, out_size)
        assert k == ksize, s
        np.testing.assert_array_equal(b, bounds, err_msg=f"bounds {s}")
        np.testing.assert_array_equal(t, kk, err_msg=f"kk {s}")


def _random_scene(seed, F, H, W, n):
    rng = np.random.default_rng(seed)
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    rgb[:, ::7] //= 3
    seg = np.zeros((F, H, W), np.uint8)
    req = []
    for i in range(n):
        f, lab = i % F, 1 + i // F
        for _ in range(int(rng.integers(1, 4))):               # a union of rectangles ...
            y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
            h, w = int(rng.integers(1, H // 3)), int(rng.integers(1, W // 3))
            seg[f, y0:y0 + h, x0:x0 + w] = lab
        ys, xs = rng.integers(0, H, 6), rng.integers(0, W, 6)   # ... and scattered pixels
        seg[f, ys, xs] = lab
        req.append((f, lab))
    return rgb, seg, req


def test_random_masks_equal_restatement(ctx):
    """two 480 x 640 frames, 40 masks (later labels overwrite earlier ones, so shapes are ragged), S = 224, chunks of 16"""
    rgb, seg, req = _random_scene(11, 2, 480, 640, 40)
    want, boxes, status = R.crops(rgb, seg, req)
    assert (status == R.OK).sum() >= 30
    z = dict(rgb=rgb, seg=seg, req=req, out_size=224)
    got = _render(ctx, z, 16, True)
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_each_side_of_the_pass_through_threshold_and_a_full_large_frame(ctx):
    """The render kernels have one size threshold: a square of side S passes through unchanged, any
    other side is resampled (upscaling below S, downscaling above).  Squares of side S - 1, S and
    S + 1, and one full-frame mask in a 1440 x 1920 frame (s = 1920, the widest table: ksize 37)."""
    from maskclustering_amd import _native
    S = 224
    rng = np.random.default_rng(2)
    rgb = rng.integers(0, 256, (1, 300, 400, 3), dtype=np.uint8)
    seg = np.zeros((1, 300, 400), np.uint8)
    for lab, side in ((1, S - 1), (2, S), (3, S + 1)):          # level-0 side = right - left
        seg[0, 10 * lab, 5] = lab
        seg[0, 10 * lab + 5, 5 + side] = lab
    req = [(0, 1), (0, 2), (0, 3)]
    prm = _native.crop_params(levels=1)
    want, boxes, status = R.crops(rgb, seg, req, levels=1)
    assert [int(b[0, 2] - b[0, 0]) for b in boxes] == [S - 1, S, S + 1] and not status.any()
    got = _render(ctx, dict(rgb=rgb, seg=seg, req=req), 2, True, prm)
    np.testing.assert_array_equal(_bits(got), _bits(want))

    big = rng.integers(0, 256, (1, 1440, 1920, 3), dtype=np.uint8)
    bseg = np.full((1, 1440, 1920), 5, np.uint8)
    bseg[0, 0, 0] = bseg[0, -1, -1] = 0                          # label 0 spans the frame through two pixels
    prm = _native.crop_params(levels=2)
    want, boxes, status = R.crops(big, bseg, [(0, 0)], levels=2)
    assert tuple(boxes[0, 1]) == (0, 0, 1920, 1440) and ctx.crop_coeffs(1920, S)[0] == 37
    got = _render(ctx, dict(rgb=big, seg=bseg, req=[(0, 0)]), 1, True, prm)
    np.testing.assert_array_equal(_bits(got), _bits(want))


def test_memory_budget_splits_a_chunk_and_bounds_one_mask(golds):
    """scratch per mask here: 3 * (131 * 32 * 3 + 32 * kmax * 4 + 32 * 8) bytes, kmax = crop_ksize(131, 32) = 19"""
    from maskclustering_amd import _native
    z = golds["clip_crops_small.npz"]
    per_mask = 3 * (131 * 32 * 3 + 32 * 19 * 4 + 32 * 8)
    own = _native.Context(0)
    try:
        own.set_memory_budget(2 * per_mask + 100)                # two masks per launch
        got = _render(own, z, 1 << 20, False)
        np.testing.assert_array_equal(_bits(got), _bits(z["want"]))
        own.set_memory_budget(per_mask - 1)
        with pytest.raises(_native.McError) as e:
            _render(own, z, 1 << 20, False)
        assert e.value.code == _native.MC_ERR_UNSUPPORTED
    finally:
        own.close()


def test_bad_arguments_return_the_library_error(ctx, golds):
    from maskclustering_amd import _native
    z = golds["clip_crops_small.npz"]
    prm = _params(z)
    for mf, ml in (([3], [1]), ([-1], [1]), ([0], [256]), ([0], [-1]), ([2 ** 32], [1])):
        with pytest.raises(_native.McError) as e:
            ctx.crop_boxes(z["seg"], mf, ml, prm)
        assert e.value.code == _native.MC_ERR_INVALID
    for bad in (dict(out_size=0), dict(levels=0), dict(out_size=-5)):
        with pytest.raises(_native.McError) as e:
            ctx.crop_boxes(z["seg"], [0], [1], _native.crop_params(**bad))
        assert e.value.code == _native.MC_ERR_INVALID
    boxes, status = ctx.crop_boxes(z["seg"], [0], [1], prm)
    with pytest.raises(_native.McError) as e:
        ctx.crop_render(z["rgb"], [3], boxes, status, prm)
    assert e.value.code == _native.MC_ERR_INVALID
    outside = boxes.copy()
    outside[0, 2, 2] = z["rgb"].shape[2] + 1
    with pytest.raises(_native.McError) as e:
        ctx.crop_render(z["rgb"], [0], outside, status, prm)
    assert e.value.code == _native.MC_ERR_INVALID


def test_iter_crops_strict_and_status(golds):
    from maskclustering_amd import _native
    from maskclustering_amd.semantics import get_open_voc_features as gf
    z = golds["clip_crops_small.npz"]
    prm = _params(z)
    ok = [r for r, s in zip(z["req"], z["status"]) if s == R.OK]
    got = np.concatenate([x.cpu().numpy() for x in gf.iter_crops(z["rgb"], z["seg"], ok, batch=4, params=prm)])
    np.testing.assert_array_equal(_bits(got), _bits(z["want"][z["status"] == R.OK]))
    for bad in ((0, 200), (0, 6)):                                # ABSENT, EMPTY
        with pytest.raises(ValueError):
            list(gf.iter_crops(z["rgb"], z["seg"], ok[:2] + [bad], params=prm))
    parts = list(gf.iter_crops(z["rgb"], z["seg"], z["req"], batch=5, params=prm, strict=False))
    got = np.concatenate([x.cpu().numpy() for x, _ in parts])
    st = np.concatenate([s.cpu().numpy() for _, s in parts])
    np.testing.assert_array_equal(st, z["status"])
    np.testing.assert_array_equal(_bits(got), _bits(z["want"]))
    assert not got[st != R.OK].any()
    for bad in ((3, 1), (0, 256)):
        with pytest.raises(_native.McError) as e:
            list(gf.iter_crops(z["rgb"], z["seg"], [bad], params=prm, strict=False))
        assert e.value.code == _native.MC_ERR_INVALID


def test_segmentation_of_another_size_goes_through_frames_decode(golds):
    """A segmentation at half the RGB size: iter_crops resizes it with mc_frames_decode and must equal the
    restatement fed with mc_frames_decode's own output.  That the decode equals cv2.INTER_NEAREST
    rests on the repository's restatement of OpenCV's resizeNN tables (tests/test_frames_decode.py),
    which no reference run pins here, as for the decode itself."""
    from maskclustering_amd import scene_pack
    from maskclustering_amd.semantics import get_open_voc_features as gf
    z = golds["clip_crops_small.npz"]
    prm = _params(z)
    H, W = z["rgb"].shape[1:3]
    small = np.ascontiguousarray(z["seg"][:, ::2, ::2][:, :45, :60])
    _, seg_full = scene_pack.decode_frames(np.zeros((3, H, W), np.uint16), small, 1000.0)
    seg_full = seg_full.cpu().numpy()
    assert seg_full.shape == (3, H, W)
    req = [(0, 1), (0, 3), (1, 7), (2, 11), (2, 0)]
    want, _, status = R.crops(z["rgb"], seg_full, req, out_size=int(z["out_size"]))
    assert not status.any()
    got = np.concatenate([x.cpu().numpy() for x in gf.iter_crops(z["rgb"], small, req, params=prm)])
    np.testing.assert_array_equal(_bits(got), _bits(want))


def _main_scene(z):
    od = {k: {"repre_mask_list": []} for k in range(int(z["num_objects"]))}
    for k, f, m in zip(z["repre_object"], z["repre_frame"], z["repre_mask"]):
        od[int(k)]["repre_mask_list"].append((int(f), int(m), 0.5))
    return od


TOL = 2 * (clip_crops_model.D + 4) * 2.0 ** -24


def test_extract_features_equals_reference_main():
    """The reference main()'s dictionary with the gather model.  The rows entering the norm are bit-equal,
    so the freedom left is the order in which the device's float32 norm sums D squares of magnitude
    <= 1 after the division, the division itself and the two adds and one division of the mean:
    atol = 2 (D + 4) 2^-24, rtol = 0."""
    from maskclustering_amd.semantics import get_open_voc_features as gf
    z = _gold("clip_crops_main.npz")
    index = {int(f): i for i, f in enumerate(z["frame_ids"])}
    pairs = gf.crop_requests(_main_scene(z))
    model = clip_crops_model.GatherModel(z["positions"])
    feats = gf.extract_features(model, z["rgb"], z["seg"], [(index[f], m) for f, m in pairs],
                                keys=[f"{f}_{m}" for f, m in pairs])
    assert sorted(feats) == list(z["keys"])
    for k, want in zip(z["keys"], z["features"]):
        assert feats[k].dtype == np.float32
        np.testing.assert_allclose(feats[k], want, rtol=0, atol=TOL)


def test_drop_in_main_writes_the_reference_file(tmp_path, monkeypatch):
    from maskclustering_amd.semantics import get_open_voc_features as gf
    z = _gold("clip_crops_main.npz")
    base = tmp_path / "objects" / "cfg"
    base.mkdir(parents=True)
    np.save(base / "object_dict.npy", _main_scene(z), allow_pickle=True)
    files = {}
    for i, f in enumerate(z["frame_ids"]):
        files[f"rgb/{int(f)}"], files[f"seg/{int(f)}"] = z["rgb"][i], z["seg"][i]
    monkeypatch.setattr(gf, "read_frame", lambda path, unchanged=False: files[path])
    ds = SimpleNamespace(object_dict_dir=str(tmp_path / "objects"), get_frame_path=lambda f: (f"rgb/{f}", f"seg/{f}"))
    gf.main(SimpleNamespace(config="cfg", seq_name_list="scene"), dataset=ds,
            model=clip_crops_model.GatherModel(z["positions"]))
    got = np.load(base / "open-vocabulary_features.npy", allow_pickle=True).item()
    assert sorted(got) == list(z["keys"])
    for k, want in zip(z["keys"], z["features"]):
        np.testing.assert_allclose(got[k], want, rtol=0, atol=TOL)


def test_run_py_command_routes_to_device(tmp_path):
    """run.py:96's `python -m semantics.get_open-voc_features --config C --seq_name_list S` in a
    reference-shaped tree with the integration hook on PYTHONPATH: the drop-in runs (its model from
    a stub open_clip in the tree, its frames through a stub cv2 in the tree) and writes the
    reference's file."""
    z = _gold("clip_crops_main.npz")
    (tmp_path / "semantics").mkdir()
    (tmp_path / "utils").mkdir()
    (tmp_path / "utils" / "__init__.py").write_text("")
    base = tmp_path / "objects" / "cfg"
    base.mkdir(parents=True)
    np.save(base / "object_dict.npy", _main_scene(z), allow_pickle=True)
    np.save(tmp_path / "positions.npy", z["positions"])
    for i, f in enumerate(z["frame_ids"]):
        np.save(tmp_path / f"rgb_{int(f)}.npy", z["rgb"][i])
        np.save(tmp_path / f"seg_{int(f)}.npy", z["seg"][i])
    (tmp_path / "utils" / "config.py").write_text(textwrap.dedent(f"""
        import argparse
        def get_args():
            p = argparse.ArgumentParser()
            p.add_argument('--config'); p.add_argument('--seq_name_list'); p.add_argument('--seq_name')
            return p.parse_args()
        class _DS:
            object_dict_dir = {str(tmp_path / "objects")!r}
            def get_frame_path(self, f):
                return {str(tmp_path)!r} + f'/rgb_{{f}}.npy', {str(tmp_path)!r} + f'/seg_{{f}}.npy'
        def get_dataset(args):
            return _DS()
    """))
    (tmp_path / "cv2.py").write_text(textwrap.dedent("""
        import numpy as np
        IMREAD_UNCHANGED, COLOR_BGR2RGB = -1, 4
        def imread(path, flag=None):
            a = np.load(path)
            return a if flag == IMREAD_UNCHANGED else a[..., ::-1].copy()
        def cvtColor(img, code):
            return img[..., ::-1].copy()
    """))
    (tmp_path / "open_clip.py").write_text(textwrap.dedent(f"""
        import sys
        import numpy as np
        sys.path.insert(0, {os.path.join(REPO, "tests")!r})
        from clip_crops_model import GatherModel
        def create_model_and_transforms(name, pretrained=None):
            return GatherModel(np.load({str(tmp_path / "positions.npy")!r})), None, None
    """))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(REPO, "integration"), REPO]))
    out = subprocess.run([sys.executable, "-m", "semantics.get_open-voc_features", "--config", "cfg", "--seq_name_list",
                          "scene"], capture_output=True, text=True, cwd=str(tmp_path), env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.load(base / "open-vocabulary_features.npy", allow_pickle=True).item()
    assert sorted(got) == list(z["keys"])
    for k, want in zip(z["keys"], z["features"]):
        np.testing.assert_allclose(got[k], want, rtol=0, atol=TOL)
