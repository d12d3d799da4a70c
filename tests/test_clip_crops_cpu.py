"""CPU checks of the CLIP crop preparation: the numpy restatement (tests/clip_crops_restatement.py)
against the fixtures made by the reference's own code (tests/golden/make_clip_crops_golden.py) and
against Pillow, the shared arithmetic of maskclustering_amd/csrc/mc_crop_plan.hpp (built stand-alone
under the address and undefined-behaviour sanitizers) against the restatement, and the request
order of the drop-in.  The GPU tests (test_gpu_clip_crops.py) compare the device path with the
same fixtures and restatement."""
import os
import subprocess

import numpy as np
import pytest

import clip_crops_restatement as R
from conftest import GOLDEN, REPO

SIDES = list(range(1, 65)) + [113, 223, 224, 225, 447, 448, 449, 777, 1000, 1440, 1920]
OUT_SIZES = (224, 32)


def _gold(name):
    return dict(np.load(os.path.join(GOLDEN, name)))


@pytest.mark.parametrize("name", ["clip_crops_small.npz", "clip_crops_224.npz"])
def test_restatement_equals_reference_fixture(name):
    z = _gold(name)
    S = int(z["out_size"])
    req = [tuple(int(v) for v in r) for r in z["requests"]]
    px, boxes, status = R.crop_pixels(z["rgb"], z["seg"], req, out_size=S)
    np.testing.assert_array_equal(status, z["status"])
    np.testing.assert_array_equal(px, z["pixels"])
    tables = R.norm_tables()
    np.testing.assert_array_equal(tables.view(np.uint32), z["tables"].view(np.uint32))
    got = R.to_float(px, status, tables)
    assert got.shape == (len(req), 3, 3, S, S) and got.dtype == np.float32
    assert not got[status != R.OK].any()


def test_small_fixture_covers_its_cases():
    z = _gold("clip_crops_small.npz")
    req = [tuple(int(v) for v in r) for r in z["requests"]]
    boxes, status = R.boxes_and_status(z["seg"], req)
    H, W = z["seg"].shape[1:]
    by = {r: boxes[i] for i, r in enumerate(req)}
    assert tuple(by[(1, 7)][2]) == (0, 0, W, H)                        # the whole frame: every clamp
    assert by[(0, 3)][1][1] == 0 and by[(0, 3)][1][3] == H             # the full height
    assert by[(0, 4)][0][2] - by[(0, 4)][0][0] == 1                    # level-0 width 1
    assert by[(0, 5)][0][2] == by[(0, 5)][0][0]                        # one pixel wide: width 0
    assert status[req.index((0, 6))] == R.EMPTY and status[req.index((0, 200))] == R.ABSENT
    assert req.count((0, 1)) == 2
    assert not z["pixels"][req.index((0, 5))].min() < 255              # an all-pad crop stays white


def test_restatement_resize_equals_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(0)
    for S in OUT_SIZES:
        for s in SIDES:
            img = rng.integers(0, 256, (s, s, 3), dtype=np.uint8)
            if s > 4:
                img[: s // 2, : s // 3] = 255
                img[s // 2:, s // 2:] = (img[s // 2:, s // 2:] // 128) * 255    # saturated steps: the clip at 0 and 255
            want = np.asarray(Image.fromarray(img).resize((S, S), Image.BICUBIC))
            np.testing.assert_array_equal(R.resize_square(img, S), want, err_msg=f"side {s} -> {S}")


def test_plan_header_equals_restatement(tmp_path):
    exe = tmp_path / "crop_plan_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(REPO, "maskclustering_amd", "csrc"),
                           os.path.join(REPO, "scripts", "crop_plan_check.cpp"), "-o", str(exe)])
    rng = np.random.default_rng(5)
    tables = [(s, S) for S in OUT_SIZES for s in SIDES]
    box_cases = []
    for _ in range(300):
        H, W = int(rng.integers(1, 2000)), int(rng.integers(1, 2000))
        l, r = sorted(int(v) for v in rng.integers(0, W, 2))
        t, b = sorted(int(v) for v in rng.integers(0, H, 2))
        box_cases.append((l, t, r, b, H, W, int(rng.integers(1, 6)), float(rng.choice([0.1, 0.0, 0.25, 0.3, 1.7]))))
    box_cases += [(0, 0, W - 1, H - 1, H, W, 3, 0.1) for H, W in ((97, 131), (1440, 1920), (1, 1))]
    text = "".join(f"T {s} {S}\n" for s, S in tables) + "".join(
        "B {} {} {} {} {} {} {} {!r}\n".format(*c) for c in box_cases)
    r = subprocess.run([str(exe)], input=text, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr[-3000:]
    lines = iter(r.stdout.splitlines())
    for s, S in tables:
        head = next(lines).split()
        ksize, bounds, kk = R.coeffs(s, S)
        assert head == ["T", str(s), str(S), str(ksize)], (s, S, head)
        got = np.array([[int(v) for v in next(lines).split()] for _ in range(S)], np.int64)
        np.testing.assert_array_equal(got[:, :2], bounds, err_msg=f"bounds {s} -> {S}")
        np.testing.assert_array_equal(got[:, 2:], kk, err_msg=f"kk {s} -> {S}")
    for l, t, r_, b, H, W, levels, e in box_cases:
        assert next(lines) == "B"
        for lv in range(levels):
            got = [int(v) for v in next(lines).split()]
            box = R.level_box((l, t, r_, b), lv, H, W, e)
            w, h = box[2] - box[0], box[3] - box[1]
            s = max(w, h)
            assert got == [*box, w, h, s, (s - w) // 2, (s - h) // 2], (l, t, r_, b, H, W, lv, e)
    assert next(lines, None) is None


def _main_object_dict(z):
    od = {k: {"repre_mask_list": []} for k in range(int(z["num_objects"]))}
    for k, f, m in zip(z["repre_object"], z["repre_frame"], z["repre_mask"]):
        od[int(k)]["repre_mask_list"].append((int(f), int(m), 0.5))
    return od


def test_crop_requests_order_and_duplicates():
    from maskclustering_amd.semantics import get_open_voc_features as gf
    z = _gold("clip_crops_main.npz")
    req = gf.crop_requests(_main_object_dict(z))
    assert req == [(int(f), int(m)) for f, m in zip(z["repre_frame"], z["repre_mask"])]
    assert len(req) > len(set(req))                                     # the duplicate is kept
    assert sorted({f"{f}_{m}" for f, m in req}) == list(z["keys"])
    # the same list from the export arrays: object 0 has masks [4, 7], object 2 [9, 1, 3, 5, 6]
    export = dict(obj_mask_off=np.array([0, 2, 2, 7]), obj_masks=np.array([4, 7, 9, 1, 3, 5, 6], np.int32),
                  obj_repre=np.array([[1, 0, -1, -1, -1], [-1] * 5, [4, 0, 2, -1, -1]], np.int32))
    col, lab = np.arange(10) % 3, np.arange(10) + 20
    got = gf.crop_requests_from_export(export, col, lab, frame_ids=[0, 10, 20])
    rows = [7, 4, 6, 9, 3]
    assert got.tolist() == [[[0, 10, 20][col[r]], lab[r]] for r in rows]


def test_restatement_reproduces_main_fixture_features():
    """the reference main()'s dictionary from the restatement's crops and :139-143 in numpy"""
    import clip_crops_model
    z = _gold("clip_crops_main.npz")
    index = {int(f): i for i, f in enumerate(z["frame_ids"])}
    pairs = [(int(f), int(m)) for f, m in zip(z["repre_frame"], z["repre_mask"])]
    x, _, status = R.crops(z["rgb"], z["seg"], [(index[f], m) for f, m in pairs], out_size=224)
    assert not status.any()
    f = x.reshape(len(pairs) * 3, -1)[:, z["positions"]]
    f = f / np.sqrt((f.astype(np.float64) ** 2).sum(axis=1, keepdims=True)).astype(np.float32)
    tol = 2 * (clip_crops_model.D + 4) * 2.0 ** -24
    for i, (fr, m) in enumerate(pairs):
        want = z["features"][list(z["keys"]).index(f"{fr}_{m}")]
        np.testing.assert_allclose(f[3 * i:3 * i + 3].mean(axis=0), want, rtol=0, atol=tol)


def test_import_does_not_parse_argv(monkeypatch):
    import importlib
    import sys
    monkeypatch.setattr(sys, "argv", ["prog", "--definitely-not-an-option"])
    mod = importlib.reload(importlib.import_module("maskclustering_amd.semantics.get_open_voc_features"))
    assert callable(mod.main) and callable(mod.iter_crops)
