"""Scene points of an RGB-D capture: the reference's ``backproject`` + ``create_downsampled_point_cloud``
(tasmap/tasmap2mct_format.py:216-284) on the device (mc_cloud_fuse_frames, include/mcgraph.h).

A TASMap scene has no mesh: its scene points are the voxel-down-sampled back-projection of every
frame, which the reference writes as ``<scene>_vh_clean_2.ply`` and reads back (dataset/tasmap.py:90-93).
``fuse_frames`` computes them from decoded frames; ``create_downsampled_point_cloud`` reads a scene
directory as the reference does; ``write_ply`` writes the file between the two reference programs.

Quirks of the reference that are kept:

* the parameter it calls ``depth_trunc=0.005`` is the VOXEL SIZE; the depth limit is hard-coded to 20 m
  (``DEPTH_LIMIT``), and Open3D drops ``d >= 20`` as well as ``d <= 0``;
* ``get_depth`` ignores the ``depth_scale`` argument of ``create_downsampled_point_cloud`` and reads a
  module global that exists only under ``__main__`` (1000).  Here the argument is used; its default is
  that 1000.

Not restated: a colour image of another size than the depth image is resized by the reference with
``cv2.INTER_LINEAR`` (:264-265); such input is refused here.  Parity-unpinned: Open3D's own summation
and output order (its hash map's; the project folds every voxel in input order and lists voxels by
first occurrence), and the PLY layout of ``write_ply``.
"""
from __future__ import annotations

import argparse
import os

import numpy as np

DEPTH_LIMIT = 20.0


def fuse_frames(depth, rgb, intrinsics, poses, voxel_size=0.005, buffer_size=10, depth_trunc=DEPTH_LIMIT, ctx=None):
    """(points float64 [n, 3], colors float64 [n, 3]) of the frames: depth float32 [F, H, W] in metres,
    rgb uint8 [F, H, W, 3], intrinsics float64 [F, 4] = fx, fy, cx, cy, poses float64 [F, 4, 4] camera ->
    world; numpy arrays, or tensors on the context's device (then the result is tensors there too).  The
    result also stays in ``ctx`` (``ctx.scene_use_cloud()`` makes it the scene's points)."""
    from . import _native

    if tuple(rgb.shape[:3]) != tuple(depth.shape):
        raise ValueError(f"colour frames of shape {tuple(rgb.shape[:3])} for depth frames of shape {tuple(depth.shape)}: "
                         "a colour image of another size than depth is not resized (the reference's cv2.INTER_LINEAR "
                         "resize is not restated)")
    own = ctx is None
    if own:
        ctx = _native.Context(0)
    try:
        prm = _native.CloudParams(float(voxel_size), float(depth_trunc), int(buffer_size))
        ctx.cloud_fuse(depth, rgb, intrinsics, poses, prm)
        on_dev = hasattr(depth, "data_ptr") and depth.device.type == "cuda"
        return ctx.cloud_get(device=on_dev)
    finally:
        if own:
            ctx.close()


def read_scene_frames(base_dir, stride=1, depth_scale=1000):
    """The frames of a scene directory as the reference lists them (:241-266): ``depth/<id>.png`` (16 bit),
    ``color/<id>.jpg``, ``pose/<id>.txt``, ``intrinsic/intrinsic_depth.txt``; ids sorted by their integer
    value, then ``[::stride]``.  Returns (frame ids, depth float32 [F, H, W], rgb uint8 [F, H, W, 3],
    intrinsics [F, 4], poses [F, 4, 4])."""
    from PIL import Image

    depth_dir = os.path.join(base_dir, "depth")
    image_list = sorted(os.listdir(depth_dir), key=lambda x: int(x.split(".")[0]))
    frame_ids = [x.split(".")[0] for x in image_list][::stride]
    intr = np.loadtxt(os.path.join(base_dir, "intrinsic", "intrinsic_depth.txt"))
    k = np.array([intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]], np.float64)
    depth, rgb, poses = [], [], []
    for fid in frame_ids:
        with Image.open(os.path.join(depth_dir, f"{fid}.png")) as im:
            raw = np.array(im)
        d = (raw.astype(np.float64) / depth_scale).astype(np.float32)  # get_depth: float64 division, then float32
        with Image.open(os.path.join(base_dir, "color", f"{fid}.jpg")) as im:
            c = np.array(im.convert("RGB"), np.uint8)
        if c.shape[:2] != d.shape:
            raise ValueError(f"frame {fid}: colour image {c.shape[1]}x{c.shape[0]}, depth image {d.shape[1]}x{d.shape[0]}: "
                             "the reference's cv2.INTER_LINEAR resize is not restated; resize the colour images first")
        depth.append(d), rgb.append(c)
        poses.append(np.loadtxt(os.path.join(base_dir, "pose", f"{fid}.txt")).reshape(4, 4))
    F = len(frame_ids)
    if F:
        if any(a.shape != depth[0].shape for a in depth):
            raise ValueError("depth images of different sizes")
        return (frame_ids, np.stack(depth), np.stack(rgb), np.tile(k, (F, 1)), np.stack(poses).astype(np.float64))
    return frame_ids, np.zeros((0, 0, 0), np.float32), np.zeros((0, 0, 0, 3), np.uint8), np.zeros((0, 4)), np.zeros((0, 4, 4))


def create_downsampled_point_cloud(base_dir, image_size=(1024, 1024), stride=1, depth_trunc=0.005, buffer_size=10,
                                   depth_scale=1000, ctx=None):
    """The reference's function of the same name and signature (:240): ``depth_trunc`` IS THE VOXEL SIZE
    (the depth limit is DEPTH_LIMIT = 20), ``image_size`` only labelled Open3D's intrinsics object and is
    not used, ``depth_scale`` divides the 16-bit depth (the reference reads a module global of that value
    instead of this argument).  Returns (points float64 [n, 3], colors float64 [n, 3])."""
    del image_size
    _, depth, rgb, intr, poses = read_scene_frames(base_dir, stride, depth_scale)
    return fuse_frames(depth, rgb, intr, poses, voxel_size=depth_trunc, buffer_size=buffer_size, ctx=ctx)


def write_ply(path, points, colors):
    """A binary little-endian PLY of ``double x y z`` and ``uchar red green blue`` per vertex, the colour
    byte ``round(clip(c, 0, 1) * 255)``: Open3D's point cloud layout as far as can be told without
    Open3D (parity-unpinned)."""
    p = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    c = np.ascontiguousarray(colors, np.float64).reshape(-1, 3)
    if len(p) != len(c):
        raise ValueError("points and colors of different lengths")
    rec = np.zeros(len(p), dtype=[("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
    rec["x"], rec["y"], rec["z"] = p[:, 0], p[:, 1], p[:, 2]
    b = np.round(np.clip(c, 0.0, 1.0) * 255.0).astype(np.uint8)
    rec["red"], rec["green"], rec["blue"] = b[:, 0], b[:, 1], b[:, 2]
    header = ("ply\nformat binary_little_endian 1.0\ncomment Created by maskclustering_amd.scene_cloud\n"
              f"element vertex {len(p)}\nproperty double x\nproperty double y\nproperty double z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def main(argv=None):
    ap = argparse.ArgumentParser(description="scene points of an RGB-D scene directory, as a PLY")
    ap.add_argument("--base_dir", required=True, help="directory with depth/, color/, pose/, intrinsic/")
    ap.add_argument("--out", required=True, help="the PLY to write (<scene>_vh_clean_2.ply)")
    ap.add_argument("--stride", type=int, default=1)
    ap.add_argument("--voxel_size", type=float, default=0.005)
    ap.add_argument("--buffer_size", type=int, default=30)
    ap.add_argument("--depth_scale", type=float, default=1000)
    a = ap.parse_args(argv)
    pts, col = create_downsampled_point_cloud(a.base_dir, stride=a.stride, depth_trunc=a.voxel_size,
                                              buffer_size=a.buffer_size, depth_scale=a.depth_scale)
    write_ply(a.out, pts, col)
    print(f"{a.out}: {len(pts)} points")


if __name__ == "__main__":
    main()
