"""Label images from a 2-D model's instance masks: the end of the reference's step 1
(mask_predict.py:94-113) on the device (mc_labels_paint, include/mcgraph.h).

The reference pulls every selected mask to the host, paints a numpy image, writes a PNG and reads it
again in ``get_segmentation``.  Here the masks stay where the model left them: ``label_image`` paints one
frame, ``label_images`` a ragged batch, and the uint8 result is a device tensor that ``frames_decode``
and ``backproject`` take as it is.  The model itself is the caller's.

The rule: an instance is selected iff ``score >= confidence_threshold`` in float32;
the selected ones are ordered by ascending score, equal scores by ascending index (torch's CPU sort
gives this order, its CUDA sort does not promise one: parity-unpinned on ties); in that order an
instance of fewer than ``min_pixels`` set pixels is skipped, every other one takes the next id from 1
and overwrites what was painted before.  A pixel is set iff its value equals 1, and the area is the
number of set pixels (the reference's ``torch.sum`` for 0/1 masks; for other values a documented
deviation).  The 256th kept instance of a frame raises ``OverflowError``, as numpy 2 does for the
reference.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np


class LabelImages(NamedTuple):
    labels: object          # uint8 [F, H, W] on the device
    num_kept: object        # int32 [F]: ids in use per frame
    label_instance: object  # int32 [F, 255]: index within its frame of the instance with id k + 1, -1 beyond
    instance_area: object   # int32 [N]: set pixels of every instance


def _raise_overflow(status):
    bad = np.flatnonzero(np.asarray(status))
    if len(bad):
        raise OverflowError(f"frame {int(bad[0])}: more than 255 instances kept, the 256th id is out of bounds for uint8")


def _cat(parts):
    if hasattr(parts[0], "data_ptr"):
        import torch
        return torch.cat(list(parts))
    return np.concatenate([np.asarray(p) for p in parts])


def label_images(frames, confidence_threshold=0.5, min_pixels=400, ctx=None) -> LabelImages:
    """The label images of a ragged batch.  ``frames``: a sequence of (pred_masks [N_f, H, W], pred_scores
    [N_f]) pairs of one image size, or a triple (masks [N, H, W], scores [N], inst_off [F + 1]) already
    concatenated.  Masks are uint8, bool or float32; tensors on the GPU or numpy arrays (all alike).
    Returns LabelImages; num_kept, label_instance and instance_area are numpy arrays.  Raises
    OverflowError naming the first frame with more than 255 kept instances."""
    from . import _native

    if len(frames) == 3 and not isinstance(frames[0], (tuple, list)) and len(getattr(frames[0], "shape", ())) == 3:
        masks, scores, off = frames
    else:
        if not len(frames):
            raise ValueError("no frames")
        off = np.concatenate([[0], np.cumsum([int(m.shape[0]) for m, _ in frames])]).astype(np.int64)
        masks, scores = _cat([m for m, _ in frames]), _cat([s for _, s in frames])
    own = ctx is None
    if own:
        ctx = _native.Context(0)
    try:
        prm = _native.paint_params(score_threshold=float(confidence_threshold), min_pixels=int(min_pixels))
        labels, status, kept, lab, area = ctx.labels_paint(masks, scores, off, prm)
    finally:
        if own:
            ctx.close()
    _raise_overflow(status)
    return LabelImages(labels, kept, lab, area)


def label_image(pred_masks, pred_scores, confidence_threshold=0.5, min_pixels=400, ctx=None):
    """The uint8 [H, W] label image of one frame, a tensor on the device: what mask_predict.py:94-113
    writes as a PNG.  pred_masks [N, H, W] (uint8, bool or float32) and pred_scores [N]: torch tensors on
    the GPU, or numpy arrays.  Raises OverflowError at the 256th kept instance."""
    return label_images([(pred_masks, pred_scores)], confidence_threshold, min_pixels, ctx).labels[0]


def to_host(labels):
    """A label tensor as a numpy uint8 array, for callers that still write PNGs."""
    return labels.detach().cpu().numpy() if hasattr(labels, "detach") else np.asarray(labels, np.uint8)
