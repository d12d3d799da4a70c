"""Numpy restatement of the CLIP crop preparation (semantics/get_open-voc_features.py:44-99 with an
open_clip-style preprocess): mask box, three level boxes, white square, Pillow's 8-bit bicubic resize
(ImagingResample: float64 coefficient set-up, 22-bit fixed-point taps, a horizontal then a vertical
pass with a uint8 intermediate), ToTensor and Normalize.  Plain Python / numpy, written for
clarity; it is the CPU statement the device path (mc_crop_*) and maskclustering_amd/csrc/mc_crop_plan.hpp
are compared with, and is itself compared with the reference's fixtures and with Pillow
(tests/test_clip_crops_cpu.py).
"""
from __future__ import annotations

import math

import numpy as np

OK, ABSENT, EMPTY = 0, 1, 2
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 22


def bicubic(t, a=-0.5):
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def coeffs(in_size, out_size):
    """(ksize, bounds int32 [out_size, 2] = (xmin, n), kk int32 [out_size, ksize]) of one axis."""
    s, S = int(in_size), int(out_size)
    scale = s / S
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ksize = 2 * int(math.ceil(support)) + 1
    bounds = np.zeros((S, 2), np.int32)
    kk = np.zeros((S, ksize), np.int32)
    for xx in range(S):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(s, int(center + support + 0.5))
        n = xmax - xmin
        w = [bicubic((x + xmin - center + 0.5) / fs) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(n):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(v * (1 << PRECISION_BITS) - 0.5) if v < 0 else int(v * (1 << PRECISION_BITS) + 0.5)
        bounds[xx] = (xmin, n)
    return ksize, bounds, kk


def _pass(img, bounds, kk):
    """one pass along axis 1 of a uint8 [rows, s, C] image -> uint8 [rows, S, C]"""
    S = len(bounds)
    out = np.zeros((img.shape[0], S, img.shape[2]), np.uint8)
    src = img.astype(np.int64)
    for xx in range(S):
        x0, n = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = (src[:, x0:x0 + n, :] * kk[xx, :n].astype(np.int64)[None, :, None]).sum(axis=1) + (1 << (PRECISION_BITS - 1))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_square(img, out_size):
    """Pillow's Image.resize((S, S), BICUBIC) of a square uint8 [s, s, C] image."""
    s = img.shape[0]
    assert img.shape[1] == s and img.dtype == np.uint8
    if s == out_size:
        return img.copy()
    _, bounds, kk = coeffs(s, out_size)
    tmp = _pass(img, bounds, kk)                                  # horizontal
    return _pass(tmp.transpose(1, 0, 2), bounds, kk).transpose(1, 0, 2)  # vertical


def mask_box(seg, label):
    """(left, top, right, bottom) of seg == label, or None when the label is absent."""
    pos = np.where(seg == label)
    if len(pos[0]) == 0:
        return None
    return int(pos[1].min()), int(pos[0].min()), int(pos[1].max()), int(pos[0].max())


def level_box(box, level, H, W, expansion=0.1):
    left, top, right, bottom = box
    if level == 0:
        return left, top, right, bottom
    x_exp = int(abs(right - left) * expansion) * level
    y_exp = int(abs(bottom - top) * expansion) * level
    return max(0, left - x_exp), max(0, top - y_exp), min(W, right + x_exp), min(H, bottom + y_exp)


def boxes_and_status(seg, requests, levels=3, expansion=0.1):
    """boxes int32 [n, levels, 4], status int32 [n] for requests (frame, label) on seg uint8 [F, H, W]."""
    _, H, W = seg.shape
    boxes = np.zeros((len(requests), levels, 4), np.int32)
    status = np.zeros(len(requests), np.int32)
    for i, (f, lab) in enumerate(requests):
        b = mask_box(seg[f], lab)
        if b is None:
            status[i] = ABSENT
            continue
        if b[0] == b[2] and b[1] == b[3]:
            status[i] = EMPTY
        for lv in range(levels):
            boxes[i, lv] = level_box(b, lv, H, W, expansion)
    return boxes, status


def square(rgb, box, pad=(255, 255, 255)):
    left, top, right, bottom = (int(v) for v in box)
    w, h = right - left, bottom - top
    s = max(w, h)
    sq = np.empty((s, s, 3), np.uint8)
    sq[:] = np.asarray(pad, np.uint8)
    ox, oy = (s - w) // 2, (s - h) // 2
    sq[oy:oy + h, ox:ox + w] = rgb[top:bottom, left:right]
    return sq


def norm_tables(mean=MEAN, std=STD):
    """float32 [3, 256]: ((float32(v) / 255f) - mean_c) / std_c"""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([(v - np.float32(mean[c])) / np.float32(std[c]) for c in range(3)]).astype(np.float32)


def crop_pixels(rgb, seg, requests, out_size=224, levels=3, expansion=0.1, pad=(255, 255, 255)):
    """uint8 [n, levels, S, S, 3] resized squares (zero where status != OK), boxes, status."""
    boxes, status = boxes_and_status(seg, requests, levels, expansion)
    px = np.zeros((len(requests), levels, out_size, out_size, 3), np.uint8)
    for i, (f, _) in enumerate(requests):
        if status[i] != OK:
            continue
        for lv in range(levels):
            px[i, lv] = resize_square(square(rgb[f], boxes[i, lv], pad), out_size)
    return px, boxes, status


def to_float(px, status, tables):
    """float32 [n, levels, 3, S, S] from the pixel indices through the 3 x 256 tables"""
    out = np.stack([tables[c][px[..., c]] for c in range(3)], axis=2).astype(np.float32)
    out[np.asarray(status) != OK] = 0
    return out


def crops(rgb, seg, requests, out_size=224, levels=3, expansion=0.1, pad=(255, 255, 255), mean=MEAN, std=STD):
    px, boxes, status = crop_pixels(rgb, seg, requests, out_size, levels, expansion, pad)
    return to_float(px, status, norm_tables(mean, std)), boxes, status
