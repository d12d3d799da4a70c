"""Drop-in for the reference's ``semantics/get_open-voc_features.py`` with the crop preparation on
the device (include/mcgraph.h, mc_crop_*).

The reference prepares, for every representative mask, three crops of its frame at growing margins,
pads each to a white square, resizes it to 224 x 224 with Pillow's bicubic filter and normalises it
(get_open-voc_features.py:44-99) in 16 DataLoader workers on the host.  Here the frames of a scene
are uploaded once, ``mc_crop_boxes`` finds every mask's boxes in one pass over the referenced
segmentation frames and ``mc_crop_render`` writes the ``[b, 3, 3, 224, 224]`` float32 batches the
model reads, bit for bit the reference's.  The CLIP model itself is the caller's (or open_clip's,
imported only when no model is given).

That open_clip's ``create_model_and_transforms("ViT-H-14", ...)`` preprocess is
``Resize(224, bicubic) -> CenterCrop -> ToTensor -> Normalize`` with the OpenAI mean / std is taken
from open_clip's documentation, not pinned by a test; size, levels, expansion, pad
colour, mean and std are parameters (``_native.crop_params``).

Importing this module does not parse ``sys.argv`` (the reference's import-time ``get_args()`` is
not copied); ``python -m semantics.get_open-voc_features`` does, through ``utils.config.get_args``.
"""
from __future__ import annotations

import os

import numpy as np

from maskclustering_amd import _device, _native  # absolute: also run as `semantics.get_open-voc_features`

CROP_SCALES = 3   # get_open-voc_features.py:18
BATCH = 64        # :132


def crop_requests(object_dict):
    """[(frame_id, mask_id)] in the reference's order (:118-129): object by object, then through
    repre_mask_list; duplicates are kept."""
    out = []
    for value in object_dict.values():
        for mask_info in value["repre_mask_list"]:
            out.append((mask_info[0], mask_info[1]))
    return out


def crop_requests_from_export(export, mask_col, mask_label, frame_ids=None):
    """The same list from an ``mc_pp_export`` result (``Context.pp_export``: obj_mask_off, obj_masks,
    obj_repre) and the scene's mask table (frame column and label of every mask-table row), as an
    int array [n, 2] with no host dictionaries: object by object, its representative masks in
    obj_repre order (-1 padding skipped).  frame_ids maps a frame column to the dataset's frame id."""
    a = {k: _device.as_numpy(export[k]) for k in ("obj_mask_off", "obj_masks", "obj_repre")}
    repre = a["obj_repre"].reshape(-1, 5)
    keep = repre >= 0
    rows = a["obj_masks"][(a["obj_mask_off"][:-1, None] + np.where(keep, repre, 0))[keep]]
    col = np.asarray(mask_col)[rows]
    frames = col if frame_ids is None else np.asarray(frame_ids)[col]
    return np.stack([frames, np.asarray(mask_label)[rows]], axis=1).astype(np.int64).reshape(-1, 2)


def _to_device_u8(a, dev):
    import torch
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a))
    if t.dtype != torch.uint8:
        raise ValueError("frames must be uint8")
    return t.to(dev).contiguous()


def iter_crops(rgb, seg, requests, batch=BATCH, params=None, strict=True):
    """Yield the model inputs of ``requests`` = [(frame index, label)] in order, ``batch`` masks at a
    time: float32 device tensors [b, levels, 3, S, S] (with strict=False: (tensor, status int32 [b])).

    rgb uint8 [F, H, W, 3] and seg uint8 [F, Hs, Ws] (numpy or tensors) are moved to the device once;
    a segmentation of another size is first resized to the RGB size as cv2.INTER_NEAREST does
    (``mc_frames_decode``; a nearest gather commutes with ``== label``, :71).  A mask whose label
    is absent from its frame (the reference's np.min raises) or covers a single pixel (its crops are
    0 x 0) raises ValueError with strict=True, before anything is rendered; with strict=False its
    rows are zeros and its status MC_CROP_ABSENT / MC_CROP_EMPTY.  An out-of-range frame index or
    label raises the library's McError and launches nothing.

    The batches are written on torch's current stream when that is not the default stream (the
    context is switched to it); on the default stream the context's own stream is waited for
    before a batch is yielded."""
    import torch
    ctx = _device.context()
    dev = ctx.torch_device
    prm = params or _native.crop_params()
    req = np.asarray(requests, np.int64).reshape(-1, 2)
    mf, ml = req[:, 0], req[:, 1]
    cur = torch.cuda.current_stream(dev)
    if cur.cuda_stream:
        ctx.set_stream(cur.cuda_stream)   # as scene_pack.decode_frames does; the context stays on it
    rgb_d = _to_device_u8(rgb, dev)
    seg_d = _to_device_u8(seg, dev)
    if rgb_d.dim() != 4 or seg_d.dim() != 3 or rgb_d.shape[0] != seg_d.shape[0]:
        raise ValueError("rgb [F, H, W, 3] and seg [F, Hs, Ws] must hold the same frames")
    F, H, W = rgb_d.shape[:3]
    if tuple(seg_d.shape[1:]) != (H, W):
        out = torch.empty((F, H, W), dtype=torch.uint8, device=dev)
        cur.synchronize()
        ctx.frames_decode(F, H, W, None, 1.0, tuple(seg_d.shape[1:]), seg_d.data_ptr(), True, None, out.data_ptr())
        seg_d = out
    boxes, status = ctx.crop_boxes(seg_d, mf, ml, prm, device=True)
    if strict:
        st = status.cpu().numpy()
        bad = np.nonzero(st != _native.MC_CROP_OK)[0]
        if len(bad):
            i = int(bad[0])
            why = "is absent from its frame" if st[i] == _native.MC_CROP_ABSENT else "covers a single pixel"
            raise ValueError(f"mask (frame {int(mf[i])}, label {int(ml[i])}) {why}")
    for i0 in range(0, len(req), int(batch)):
        i1 = min(len(req), i0 + int(batch))
        x = ctx.crop_render(rgb_d, mf[i0:i1], boxes[i0:i1], status[i0:i1], prm)
        yield x if strict else (x, status[i0:i1])


def extract_features(model, rgb, seg, requests, keys=None, batch=BATCH, params=None):
    """get_open-voc_features.py:135-143: {f"{frame}_{label}": float32 feature} of the requests.  The
    crops go through ``model.encode_image`` as [b * levels, 3, S, S], every row is divided by its
    norm, and a mask's feature is the float32 mean of its rows, ((r0 + r1) + r2) / 3 as
    np.mean(axis=0) sums them.  keys: the dictionary key of every request (default
    f"{frame index}_{label}"); a later duplicate overwrites an earlier one."""
    import torch
    prm = params or _native.crop_params()
    req = np.asarray(requests, np.int64).reshape(-1, 2)
    if keys is None:
        keys = [f"{int(f)}_{int(m)}" for f, m in req]
    S, L = int(prm.out_size), int(prm.levels)
    feats = {}
    i0 = 0
    for x in iter_crops(rgb, seg, req, batch=batch, params=prm, strict=True):
        with torch.no_grad():
            f = model.encode_image(x.reshape(-1, 3, S, S)).float()
            f = f / f.norm(dim=-1, keepdim=True)
            f = f.reshape(x.shape[0], L, -1)
            mean = f[:, 0]
            for lv in range(1, L):
                mean = mean + f[:, lv]
            mean = (mean / L).cpu().numpy()
        for j in range(x.shape[0]):
            feats[keys[i0 + j]] = mean[j]
        i0 += x.shape[0]
    return feats


def read_frame(path, unchanged=False):
    """One image file as the reference reads it (:90-93): RGB uint8 [H, W, 3], or with unchanged the
    stored array (the segmentation).  cv2 when it is importable, otherwise Pillow.  Replaceable:
    ``main`` calls ``get_open_voc_features.read_frame``."""
    try:
        import cv2
    except ImportError:
        from PIL import Image
        with Image.open(path) as im:
            return np.asarray(im if unchanged else im.convert("RGB"))
    if unchanged:
        return cv2.imread(path, cv2.IMREAD_UNCHANGED)
    return cv2.cvtColor(cv2.imread(path), cv2.COLOR_BGR2RGB)


def load_clip():
    """:101-107 (open_clip is imported only here)"""
    import open_clip
    model, _, _preprocess = open_clip.create_model_and_transforms("ViT-H-14", pretrained="laion2b_s32b_b79k")
    model.cuda()
    model.eval()
    return model


def main(args=None, dataset=None, model=None):
    """get_open-voc_features.py:109-149 for ``args.seq_name_list`` ('+'-separated; or ``args.seq_name``):
    writes ``<object_dict_dir>/<config>/open-vocabulary_features.npy`` per scene.  dataset: the scene's
    dataset object (default: the reference's ``utils.config.get_dataset``); model: anything with
    ``encode_image`` (default: open_clip's ViT-H-14)."""
    if args is None:
        from utils.config import get_args
        args = get_args()
    if model is None:
        model = load_clip()
    names = getattr(args, "seq_name_list", None) or args.seq_name
    for seq_name in str(names).split("+"):
        args.seq_name = seq_name
        ds = dataset
        if ds is None:
            from utils.config import get_dataset
            ds = get_dataset(args)
        base = os.path.join(ds.object_dict_dir, args.config)
        object_dict = np.load(os.path.join(base, "object_dict.npy"), allow_pickle=True).item()
        pairs = crop_requests(object_dict)
        frame_ids = list(dict.fromkeys(f for f, _ in pairs))        # first-use order
        index = {f: i for i, f in enumerate(frame_ids)}
        feats = {}
        if pairs:
            rgbs, segs = [], []
            for f in frame_ids:
                rgb_path, seg_path = ds.get_frame_path(f)
                rgbs.append(read_frame(rgb_path))
                segs.append(_device.seg_u8(read_frame(seg_path, unchanged=True)))
            req = [(index[f], m) for f, m in pairs]
            keys = [f"{f}_{m}" for f, m in pairs]
            feats = extract_features(model, np.stack(rgbs), np.stack(segs), req, keys=keys)
        np.save(os.path.join(base, "open-vocabulary_features.npy"), feats)


if __name__ == "__main__":  # python -m semantics.get_open-voc_features --config ... (run.py)
    main()
