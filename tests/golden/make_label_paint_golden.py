"""Makes tests/golden/label_paint_golden.npz: label images painted by the reference's own
mask_predict.py ``__main__`` block, executed unmodified (runpy) with stand-in modules for detectron2,
mask2former, predictor and cv2.  ``VisualizationDemo.run_on_image`` returns synthetic pred_masks / scores
as CPU torch tensors, ``cv2.imwrite`` is captured, the image list is empty files in a temporary directory.

Run only where the reference exists:  python tests/golden/make_label_paint_golden.py <reference dir>

The fixture is data only: per frame the masks bit-packed (value == 1), their dtype as given to the
reference, the float32 scores, the threshold of the run and the captured uint8 image.  Cases: overlapping
instances in rank order, a kept instance fully covered by higher ranks, areas of exactly 399 and 400,
scores at the threshold, one float32 ulp below it, NaN and +inf, a frame where nothing is selected, a
pair of tied scores (asserted below to be ordered by ascending index by torch's CPU sort), a threshold
of 0.7 (float32(0.7) < 0.7, yet a score of float32(0.7) is selected), 48 x 40 and 64 x 64 frames.
"""
import os
import runpy
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from label_paint_restatement import paint_frame  # noqa: E402


def rect(H, W, y0, y1, x0, x1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x0:x1] = 1
    return m


def frames_050():
    """the run at the default threshold 0.5: (masks uint8 [N, H, W], scores float32 [N], dtype name)"""
    f32 = np.float32
    out = []
    H, W = 48, 40
    below = np.nextafter(f32(0.5), f32(0))
    # overlapping in rank order; instance 2 (kept, 20 x 20) is fully covered by instances 0 and 4, which rank higher
    m = [rect(H, W, 0, 30, 0, 30), rect(H, W, 10, 40, 10, 40), rect(H, W, 5, 25, 5, 25), rect(H, W, 20, 48, 0, 20),
         rect(H, W, 0, 28, 0, 28)]
    out.append((np.stack(m), np.array([0.9, 0.6, 0.55, 0.7, 0.95], f32), "float32"))
    # areas of exactly 399 and 400 (one pixel cleared from a 20 x 20 square), both selected
    a399 = rect(H, W, 2, 22, 3, 23)
    a399[2, 3] = 0
    m = [a399, rect(H, W, 20, 40, 15, 35), rect(H, W, 0, 48, 0, 40)]
    out.append((np.stack(m), np.array([0.99, 0.8, 0.6], f32), "float32"))
    # scores at the threshold, one ulp below it, NaN and +inf
    m = [rect(H, W, 0, 24, 0, 24), rect(H, W, 12, 36, 12, 36), rect(H, W, 24, 48, 0, 40), rect(H, W, 6, 30, 16, 40)]
    out.append((np.stack(m), np.array([0.5, below, np.nan, np.inf], f32), "float32"))
    # nothing selected
    out.append((np.stack([rect(H, W, 0, 48, 0, 40), rect(H, W, 0, 24, 0, 24)]), np.array([0.49, below], f32), "uint8"))
    # a pair of tied scores (instances 1 and 3) that overlap, between two others
    m = [rect(H, W, 0, 25, 0, 25), rect(H, W, 10, 35, 10, 35), rect(H, W, 30, 48, 0, 40), rect(H, W, 15, 40, 5, 30)]
    out.append((np.stack(m), np.array([0.6, 0.75, 0.9, 0.75], f32), "float32"))
    # 64 x 64: random discs, small ones among them, float32 and bool masks
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:64]
    for dtype in ("float32", "bool", "uint8"):
        n = 12
        c, r = rng.uniform(0, 64, (n, 2)), rng.uniform(6, 24, n)
        m = np.stack([((yy - c[i, 0]) ** 2 + (xx - c[i, 1]) ** 2 <= r[i] ** 2).astype(np.uint8) for i in range(n)])
        out.append((m, rng.uniform(0.2, 1.0, n).astype(f32), dtype))
    return out


def frames_070():
    """the run at threshold 0.7: float32(0.7) is selected, one ulp below is not"""
    f32 = np.float32
    H, W = 48, 40
    t = f32(0.7)
    m = [rect(H, W, 0, 24, 0, 24), rect(H, W, 12, 36, 12, 36), rect(H, W, 24, 48, 0, 40), rect(H, W, 6, 30, 16, 40)]
    s = np.array([t, np.nextafter(t, f32(0)), np.nextafter(t, f32(1)), 0.95], f32)
    return [(np.stack(m), s, "float32")]


def run_reference(ref_dir, frames, threshold):
    """the images mask_predict.py writes for the frames, in order"""
    captured = {}
    tdt = {"float32": torch.float32, "bool": torch.bool, "uint8": torch.uint8}

    class Demo:
        def __init__(self, cfg):
            pass

        def run_on_image(self, img):
            masks, scores, dtype = frames[img]
            inst = types.SimpleNamespace(pred_masks=torch.from_numpy(masks.copy()).to(tdt[dtype]),
                                         scores=torch.from_numpy(scores.copy()))
            return {"instances": inst}

    class Cfg:
        def merge_from_file(self, f):
            pass

        def merge_from_list(self, l):
            pass

        def freeze(self):
            pass

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        return m

    def imwrite(path, image):
        captured[int(os.path.basename(path).split(".")[0])] = np.array(image, copy=True)
        return True

    stand_ins = {
        "cv2": mod("cv2", imwrite=imwrite),
        "detectron2": mod("detectron2"),
        "detectron2.config": mod("detectron2.config", get_cfg=lambda: Cfg()),
        "detectron2.data": mod("detectron2.data"),
        "detectron2.data.detection_utils": mod("detectron2.data.detection_utils",
                                               read_image=lambda path, format=None: int(os.path.basename(path).split(".")[0])),
        "detectron2.projects": mod("detectron2.projects"),
        "detectron2.projects.deeplab": mod("detectron2.projects.deeplab", add_deeplab_config=lambda cfg: None),
        "mask2former": mod("mask2former", add_maskformer2_config=lambda cfg: None),
        "predictor": mod("predictor", VisualizationDemo=Demo),
    }
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stand_ins["tqdm"] = mod("tqdm", tqdm=lambda it, **kw: it)
    saved = {k: sys.modules.get(k) for k in stand_ins}
    argv = sys.argv
    with tempfile.TemporaryDirectory() as root:
        os.makedirs(os.path.join(root, "seq", "color"))
        for k in range(len(frames)):
            open(os.path.join(root, "seq", "color", f"{k:04d}.jpg"), "w").close()
        sys.modules.update(stand_ins)
        sys.argv = ["mask_predict.py", "--seq_name_list", "seq", "--root", root, "--image_path_pattern", "color/*.jpg",
                    "--dataset", "scannet", "--confidence-threshold", repr(threshold)]
        try:
            runpy.run_path(os.path.join(ref_dir, "mask_predict.py"), run_name="__main__")
        finally:
            sys.argv = argv
            for k, v in saved.items():
                if v is None:
                    sys.modules.pop(k, None)
                else:
                    sys.modules[k] = v
    assert sorted(captured) == list(range(len(frames))), sorted(captured)
    return [captured[k] for k in range(len(frames))]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref_dir = sys.argv[1]
    data, k = {}, 0
    for threshold, frames in ((0.5, frames_050()), (0.7, frames_070())):
        images = run_reference(ref_dir, frames, threshold)
        for (masks, scores, dtype), image in zip(frames, images):
            assert image.dtype == np.uint8 and image.shape == masks.shape[1:]
            data[f"f{k}_bits"] = np.packbits(masks.reshape(len(masks), -1) == 1, axis=1, bitorder="little")
            data[f"f{k}_shape"] = np.array(masks.shape[1:], np.int32)
            data[f"f{k}_scores"] = scores
            data[f"f{k}_dtype"] = np.array(dtype)
            data[f"f{k}_threshold"] = np.array(threshold, np.float64)
            data[f"f{k}_image"] = image
            k += 1
    data["num_frames"] = np.array(k, np.int32)
    # the tie (frame 4, instances 1 and 3): the reference painted index 1 before index 3
    tie = data["f4_image"]
    want, kept, _ = paint_frame(frames_050()[4][0], frames_050()[4][1])
    assert list(kept) == [0, 1, 3, 2] and tie[20, 20] == 3 and np.array_equal(tie, want), "tie not ordered by ascending index"
    out = os.path.join(HERE, "label_paint_golden.npz")
    np.savez_compressed(out, **data)
    print(f"{out}: {k} frames, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
