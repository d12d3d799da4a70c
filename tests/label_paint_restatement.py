"""The label image of one frame's instance masks, restated in numpy from the reference's
mask_predict.py:94-113 (the contract of mc_labels_paint, include/mcgraph.h):

1. instance i is selected iff float32(score[i]) >= float32(threshold) (torch casts the Python scalar
   to the tensor's dtype; a NaN score never is);
2. the selected instances are ordered by ascending score with a STABLE sort: equal scores, -0.0 and
   +0.0 included, by ascending instance index;
3. in that order an instance whose area is < min_pixels is skipped and takes no id; every other one
   takes the next id from 1 and sets its pixels to it, later ones overwriting earlier ones;
4. a pixel is set iff its value equals 1; the area is the number of set pixels of the whole mask;
5. the 256th kept instance overflows uint8: OverflowError from ``paint_frame``, and from
   ``paint_frames`` status 1 (MC_PAINT_OVERFLOW), an all-zero image and a label_instance row of -1.
"""
import numpy as np

PAINT_OK, PAINT_OVERFLOW = 0, 1
MAX_IDS = 255


def load_golden():
    """The frames of tests/golden/label_paint_golden.npz (made by the reference's own program,
    tests/golden/make_label_paint_golden.py): dicts of masks (the dtype the reference was given),
    scores, threshold and the image it wrote."""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "label_paint_golden.npz"))
    frames = []
    for k in range(int(g["num_frames"])):
        H, W = (int(x) for x in g[f"f{k}_shape"])
        bits = np.unpackbits(g[f"f{k}_bits"], axis=1, bitorder="little")[:, :H * W]
        frames.append(dict(masks=bits.reshape(-1, H, W).astype(str(g[f"f{k}_dtype"])), scores=g[f"f{k}_scores"],
                           threshold=float(g[f"f{k}_threshold"]), image=g[f"f{k}_image"]))
    return frames


def plan_frame(masks, scores, threshold=0.5, min_pixels=400):
    """(kept instance indices in paint order, area int32 [N]) of masks [N, H, W], scores [N]"""
    masks = np.asarray(masks)
    scores = np.asarray(scores, np.float32).reshape(-1)
    n = len(scores)
    area = (masks.reshape(n, -1) == 1).sum(axis=1).astype(np.int32) if n else np.zeros(0, np.int32)
    with np.errstate(invalid="ignore"):
        selected = np.flatnonzero(scores >= np.float32(threshold))
    ranks = selected[np.argsort(scores[selected], kind="stable")]
    kept = np.array([i for i in ranks if area[i] >= min_pixels], np.int64)
    return kept, area


def paint_frame(masks, scores, threshold=0.5, min_pixels=400):
    """(image uint8 [H, W], kept instance indices in id order, area) of one frame; OverflowError at the
    256th kept instance, as numpy 2 raises it for the reference"""
    masks = np.asarray(masks)
    kept, area = plan_frame(masks, scores, threshold, min_pixels)
    image = np.zeros(masks.shape[1:], np.uint8)
    for k, i in enumerate(kept):
        if k + 1 > MAX_IDS:
            raise OverflowError(f"Python integer {k + 1} out of bounds for uint8")
        image[masks[i] == 1] = k + 1
    return image, kept, area


def paint_frames(masks, scores, inst_off, threshold=0.5, min_pixels=400):
    """dict(labels uint8 [F, H, W], status, num_kept int32 [F], label_instance int32 [F, 255],
    instance_area int32 [N]) of a ragged batch: what mc_labels_paint returns"""
    masks = np.asarray(masks)
    scores = np.asarray(scores, np.float32).reshape(-1)
    inst_off = np.asarray(inst_off, np.int64)
    F = len(inst_off) - 1
    out = dict(labels=np.zeros((F,) + masks.shape[1:], np.uint8), status=np.zeros(F, np.int32),
               num_kept=np.zeros(F, np.int32), label_instance=np.full((F, MAX_IDS), -1, np.int32),
               instance_area=np.zeros(len(scores), np.int32))
    for f in range(F):
        a, b = int(inst_off[f]), int(inst_off[f + 1])
        kept, area = plan_frame(masks[a:b], scores[a:b], threshold, min_pixels)
        out["instance_area"][a:b] = area
        out["num_kept"][f] = len(kept)
        if len(kept) > MAX_IDS:
            out["status"][f] = PAINT_OVERFLOW
            continue
        out["label_instance"][f, :len(kept)] = kept
        for k, i in enumerate(kept):
            out["labels"][f][masks[a + i] == 1] = k + 1
    return out
