"""Golden fixtures for the CLIP crop preparation (mc_crop_*): the REFERENCE's own
``semantics/get_open-voc_features.py`` run on synthetic frames, its outputs captured.

Run ONLY in the build container, where /root/reference exists:

    python tests/golden/make_clip_crops_golden.py

The reference module is loaded from its file, unmodified, with stand-ins for what this container
lacks: ``cv2`` (imread serves the synthetic frames from memory, as BGR like OpenCV; cvtColor swaps
the channels back; resize with INTER_NEAREST is served for EQUAL sizes only, asserted, where it is
the identity), ``open_clip`` (create_model_and_transforms returns the gather model of
tests/clip_crops_model.py and a preprocess built from Pillow and torch: Resize(S, bicubic) of a
square image, ToTensor, Normalize with open_clip's OpenAI mean / std; CenterCrop of an S x S image
is the identity) and ``utils.config`` (get_args / get_dataset serving the synthetic scene).

Stored (data only):
  clip_crops_small.npz   S = 32, three 97 x 131 frames, the masks listed in make_small(); the output
                         of CroppedImageDataset.__getitem__ for every request
  clip_crops_224.npz     S = 224, one mask in a 260 x 340 frame: level 0 is near scale 1 (side 225),
                         levels 1 and 2 downscale
  clip_crops_main.npz    the feature dictionary main() writes, driven whole (DataLoader with its 16
                         workers included) with the gather model and Tensor.cuda patched to the identity
Outputs are stored as uint8 pixel indices [n, 3, S, S, 3] plus the 3 x 256 float32 tables; the maker
asserts that tables[c][index] reproduces the reference's float32 bits exactly.  Two requests have
no crop: a label absent from its frame, on which __getitem__ raises (np.min of an empty array;
status 1), and a single-pixel mask, whose 0 x 0 square the installed Pillow resizes to an all-black
image (asserted; status 2: the device path reports it instead of rendering nothing into black).
Their pixels are stored as zeros and the device's rows for them are zeros.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import clip_crops_model  # noqa: E402
import clip_crops_restatement as R  # noqa: E402

REF = "/root/reference"
FILES = {}          # path -> array served by the cv2 stand-in
STATE = {"size": 224, "model": None}


def _preprocess(im):
    import torch
    from PIL import Image
    S = STATE["size"]
    assert im.size[0] == im.size[1]
    im = im.resize((S, S), Image.BICUBIC)                                            # Resize(S, bicubic); CenterCrop: identity
    x = torch.from_numpy(np.asarray(im).copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)   # ToTensor
    mean = torch.as_tensor(R.MEAN, dtype=torch.float32)[:, None, None]
    std = torch.as_tensor(R.STD, dtype=torch.float32)[:, None, None]
    return x.sub_(mean).div_(std)                                                    # Normalize


def _install_stubs(args, dataset):
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST, cv2.COLOR_BGR2RGB, cv2.IMREAD_UNCHANGED = 0, 4, -1

    def imread(path, flag=None):
        a = FILES[path]
        return a.copy() if flag == cv2.IMREAD_UNCHANGED else a[..., ::-1].copy()

    def cvt(img, code):
        assert code == cv2.COLOR_BGR2RGB
        return img[..., ::-1].copy()

    def resize(img, dsize, interpolation=None):
        assert interpolation == cv2.INTER_NEAREST and (img.shape[1], img.shape[0]) == tuple(dsize), "equal sizes only"
        return img.copy()

    cv2.imread, cv2.cvtColor, cv2.resize = imread, cvt, resize
    oc = types.ModuleType("open_clip")
    oc.create_model_and_transforms = lambda *a, **k: (STATE["model"], None, _preprocess)
    utils = types.ModuleType("utils")
    cfg = types.ModuleType("utils.config")
    cfg.get_args = lambda: args
    cfg.get_dataset = lambda a: dataset
    utils.config = cfg
    sys.modules.update({"cv2": cv2, "open_clip": oc, "utils": utils, "utils.config": cfg})


def _load_reference():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_get_open_voc_features",
                                                  os.path.join(REF, "semantics", "get_open-voc_features.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _frames(rng, F, H, W, noise):
    """structured-plus-random RGB: two gradients and a checker, plus noise on a fraction of the pixels"""
    y, x = np.mgrid[0:H, 0:W]
    rgb = np.zeros((F, H, W, 3), np.int64)
    for f in range(F):
        rgb[f, ..., 0] = (x * 255) // max(W - 1, 1)
        rgb[f, ..., 1] = (y * 255) // max(H - 1, 1)
        rgb[f, ..., 2] = (((x // 8) + (y // 8) + f) % 2) * 200 + 20
    n = rng.integers(-60, 61, rgb.shape)
    n[rng.random(rgb.shape[:3]) > noise] = 0
    return np.clip(rgb + n, 0, 255).astype(np.uint8)


def make_small(rng):
    H, W = 97, 131
    seg = np.zeros((3, H, W), np.uint8)
    seg[0, 10:40, 20:70] = 1                                   # a plain rectangle
    for r in range(50, 81):
        seg[0, r, 5:6 + (r - 50)] = 2                          # a triangle: its box is larger than its pixels
    seg[0, :, 100:111] = 3                                     # the full height
    seg[0, 45:48, 80:82] = 4                                   # 3 x 2: level-0 width 1
    seg[0, 60:76, 90] = 5                                      # one pixel wide: an all-pad crop
    seg[0, 85, 95] = 6                                         # a single pixel: EMPTY
    seg[1] = 7                                                 # a whole frame: every clamp applies
    seg[2, 0:10, 0:15] = 8                                     # the four corners
    seg[2, 0:8, 120:131] = 9
    seg[2, 90:97, 0:12] = 10
    seg[2, 85:97, 115:131] = 11
    req = [(0, 1), (0, 2), (0, 3), (1, 7), (2, 8), (2, 9), (2, 10), (2, 11), (0, 4), (0, 5), (0, 6), (0, 200), (0, 1),
           (2, 0)]
    status = [0] * len(req)
    status[10], status[11] = R.EMPTY, R.ABSENT
    return _frames(rng, 3, H, W, 0.5), seg, req, status


def make_224(rng):
    H, W = 260, 340
    seg = np.zeros((1, H, W), np.uint8)
    seg[0, 30:201, 50:276] = 9                                 # right - left = 225, bottom - top = 170
    seg[0, 30:100, 50:120] = 0                                 # not a rectangle
    seg[0, 30, 50] = 9
    seg[0, 200, 275] = 9
    return _frames(rng, 1, H, W, 0.15), seg, [(0, 9)], [0]


def _to_indices(x, tables):
    """float32 [levels, 3, S, S] -> uint8 [levels, S, S, 3], asserting exact float bits"""
    x = x.numpy()
    idx = np.zeros(x.shape[:1] + x.shape[2:] + (3,), np.uint8)
    for c in range(3):
        t = tables[c]
        assert np.all(np.diff(t) > 0)
        i = np.searchsorted(t, x[:, c])
        assert i.max() < 256 and np.array_equal(t[i].view(np.uint32), x[:, c].view(np.uint32)), "not a table value"
        idx[..., c] = i
    return idx


def run_getitem(mod, rgb, seg, req, want_status, S, levels=3):
    STATE["size"] = S
    FILES.clear()
    for f in range(len(rgb)):
        FILES[f"rgb/{f}"], FILES[f"seg/{f}"] = rgb[f], seg[f]
    ds = mod.CroppedImageDataset(["scene"] * len(req), [f for f, _ in req], [m for _, m in req],
                                 [f"rgb/{f}" for f, _ in req], [f"seg/{f}" for f, _ in req], _preprocess)
    tables = R.norm_tables()
    px = np.zeros((len(req), levels, S, S, 3), np.uint8)
    for i in range(len(req)):
        try:
            x, _, fid, mid = ds[i]
        except Exception as e:  # noqa: BLE001  (whatever numpy / Pillow raise on an absent label or a 0 x 0 crop)
            assert want_status[i] != R.OK, (i, req[i], repr(e))
            print(f"  request {i} {req[i]}: status {want_status[i]} ({type(e).__name__}: {e})")
            continue
        assert (fid, mid) == tuple(req[i]) and tuple(x.shape) == (levels, 3, S, S), (i, req[i], tuple(x.shape))
        idx = _to_indices(x, tables)
        if want_status[i] == R.EMPTY:   # Pillow resizes the 0 x 0 square to black; the device path reports EMPTY instead
            assert not idx.any(), (i, req[i])
            print(f"  request {i} {req[i]}: status {R.EMPTY} (a 0 x 0 square; Pillow resizes it to black)")
            continue
        assert want_status[i] == R.OK, (i, req[i])
        px[i] = idx
    return px, tables


def run_main(mod, tmp):
    """main() whole, at its fixed 224: two 60 x 80 frames with the dataset's frame ids 0 and 10"""
    import torch
    rng = np.random.default_rng(3)
    H, W = 60, 80
    rgb = _frames(rng, 2, H, W, 0.5)
    seg = np.zeros((2, H, W), np.uint8)
    seg[0, 5:30, 10:50] = 1
    seg[0, 35:55, 20:75] = 2
    seg[1, 0:60, 30:60] = 3
    seg[1, 10:22, 2:20] = 4
    frame_ids = [0, 10]
    od = {0: {"repre_mask_list": [(0, 1, 0.9), (10, 3, 0.8)]},
          1: {"repre_mask_list": []},
          2: {"repre_mask_list": [(10, 4, 0.7), (0, 1, 0.6), (0, 2, 0.5)]}}
    FILES.clear()
    for k, f in enumerate(frame_ids):
        FILES[f"rgb/{f}"], FILES[f"seg/{f}"] = rgb[k], seg[k]
    obj_dir = os.path.join(tmp, "objects")
    os.makedirs(os.path.join(obj_dir, "cfg"))
    np.save(os.path.join(obj_dir, "cfg", "object_dict.npy"), od, allow_pickle=True)
    mod.args.seq_name_list, mod.args.config = "scene", "cfg"
    ds = sys.modules["utils.config"].get_dataset(None)
    ds.object_dict_dir = obj_dir
    ds.get_frame_path = lambda f: (f"rgb/{f}", f"seg/{f}")
    STATE["size"] = 224
    pos = clip_crops_model.gather_positions(224)
    STATE["model"] = clip_crops_model.GatherModel(pos)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        mod.main()
    finally:
        torch.Tensor.cuda = cuda
    feats = np.load(os.path.join(obj_dir, "cfg", "open-vocabulary_features.npy"), allow_pickle=True).item()
    keys = sorted(feats)
    repre = [(k, f, m) for k, v in od.items() for f, m, _ in v["repre_mask_list"]]
    return dict(rgb=rgb, seg=seg, frame_ids=np.array(frame_ids), positions=pos, num_objects=np.array(len(od)),
                repre_object=np.array([r[0] for r in repre]), repre_frame=np.array([r[1] for r in repre]),
                repre_mask=np.array([r[2] for r in repre]), keys=np.array(keys),
                features=np.stack([feats[k] for k in keys]).astype(np.float32))


def _save(name, **arrays):
    path = os.path.join(HERE, name)
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    assert size < 600_000, (name, size)
    print(f"{name}: {size / 1e3:.1f} kB")


def main():
    args = SimpleNamespace(seq_name_list="scene", config="cfg", seq_name="scene")
    _install_stubs(args, SimpleNamespace())
    mod = _load_reference()
    assert mod.CROP_SCALES == 3
    for name, maker, S, seed in (("clip_crops_small.npz", make_small, 32, 1), ("clip_crops_224.npz", make_224, 224, 2)):
        rgb, seg, req, status = maker(np.random.default_rng(seed))
        print(name)
        px, tables = run_getitem(mod, rgb, seg, req, status, S)
        _save(name, rgb=rgb, seg=seg, requests=np.array(req, np.int32), status=np.array(status, np.int32), pixels=px,
              tables=tables, out_size=np.array(S))
    with tempfile.TemporaryDirectory() as tmp:
        _save("clip_crops_main.npz", **run_main(mod, tmp))


if __name__ == "__main__":
    main()
