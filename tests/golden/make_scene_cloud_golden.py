"""Golden fixture for the scene point cloud fusion from the REFERENCE's own function.

Run ONLY where the reference checkout exists (REF below):

    python tests/golden/make_scene_cloud_golden.py

``tasmap/tasmap2mct_format.py`` is imported unmodified and its ``create_downsampled_point_cloud`` runs
on a small temporary scene directory.  Open3D, cv2 and imageio are absent here (tqdm is stubbed too
when absent), so the calls the function makes are served by stubs: the image readers by Pillow, the
Open3D calls (Image, RGBDImage.create_from_color_and_depth, PointCloud.create_from_rgbd_image,
transform, +=, voxel_down_sample, clear, PinholeCameraIntrinsic) by tests/scene_cloud_restatement.py.
The module's ``depth_scale`` global, which exists only under ``__main__`` there, is set to 1000.

So the fixture pins the reference's GLUE exactly: the frame order (integer value of the file name), the
stride, the flush rule, the remainder, the final pass, the intrinsics it reads from the matrix, the
float32 depth; and the library semantics only as restated (parity-unpinned there: DESIGN.md §5).

The fixture holds data only: the decoded arrays of every file of the scene directory (in os.listdir's
string order, with the names) and the function's result.  No source is copied.
"""
from __future__ import annotations

import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))

import scene_cloud_restatement as R  # noqa: E402


class _Image:
    def __init__(self, a):
        self.a = np.asarray(a)


class _RGBD:
    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
        assert depth_scale == 1.0 and not convert_rgb_to_intensity
        r = _RGBD()
        r.color, r.depth, r.trunc = color.a, depth.a, float(depth_trunc)
        return r


class _Intrinsic:
    def set_intrinsics(self, w, h, fx, fy, cx, cy):
        self.k = np.array([fx, fy, cx, cy], np.float64)


class _PointCloud:
    def __init__(self):
        self.points, self.colors = np.zeros((0, 3)), np.zeros((0, 3))
        self._pending = None

    @staticmethod
    def create_from_rgbd_image(rgbd, intr):
        p = _PointCloud()
        p._pending = (rgbd, intr)  # camera points and pose are one expression in the restatement: done at transform
        return p

    def transform(self, T):
        rgbd, intr = self._pending
        self.points, self.colors = R.frame_points(rgbd.depth, rgbd.color, intr.k, T, rgbd.trunc)
        self._pending = None
        return self

    def __iadd__(self, o):
        assert o._pending is None
        self.points = np.concatenate([self.points, o.points])
        self.colors = np.concatenate([self.colors, o.colors])
        return self

    def voxel_down_sample(self, voxel_size):
        out = _PointCloud()
        out.points, out.colors, _ = R.voxel_down_sample(self.points, self.colors, voxel_size)
        return out

    def clear(self):
        self.points, self.colors = np.zeros((0, 3)), np.zeros((0, 3))
        return self


def _pil_read(path, *a, **k):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def _import_reference():
    sys.dont_write_bytecode = True
    o3d = types.ModuleType("open3d")
    o3d.geometry = types.SimpleNamespace(Image=_Image, RGBDImage=_RGBD, PointCloud=_PointCloud)
    o3d.camera = types.SimpleNamespace(PinholeCameraIntrinsic=_Intrinsic)
    sys.modules["open3d"] = o3d
    cv2 = types.ModuleType("cv2")
    cv2.imread = _pil_read
    cv2.INTER_LINEAR = 1

    def _no_resize(*a, **k):
        raise AssertionError("the fixture's colour images have the depth images' size")
    cv2.resize = _no_resize
    sys.modules["cv2"] = cv2
    imageio = types.ModuleType("imageio")
    imageio.v2 = types.SimpleNamespace(imread=_pil_read)
    sys.modules["imageio"] = imageio
    try:
        import tqdm  # noqa: F401
    except ImportError:
        tq = types.ModuleType("tqdm")

        class _Bar:
            def __init__(self, *a, **k):
                pass

            def __enter__(self):
                return self

            def __exit__(self, *a):
                return False

            def set_description(self, *a):
                pass

            def update(self, *a):
                pass
        tq.tqdm = _Bar
        sys.modules["tqdm"] = tq
    sys.path.insert(0, os.path.join(REF, "tasmap"))
    import tasmap2mct_format as mod
    mod.depth_scale = 1000  # the global get_depth reads; it exists only under __main__ there
    return mod


IDS = [10, 2, 33, 4, 5, 21, 8]  # string order and integer order differ
STRIDE, BUFFER, VOXEL = 2, 3, 0.05
H, W = 24, 32


def make_scene(base):
    from PIL import Image
    depth, rgb, K, T = R.synthetic_frames(len(IDS), H, W, seed=11)
    for sub in ("depth", "color", "pose", "intrinsic"):
        os.makedirs(os.path.join(base, sub))
    m = np.eye(4)
    m[0, 0], m[1, 1], m[0, 2], m[1, 2] = K[0]
    np.savetxt(os.path.join(base, "intrinsic", "intrinsic_depth.txt"), m)
    for k, fid in enumerate(IDS):
        d16 = np.round(depth[k].astype(np.float64) * 1000).astype(np.uint16)
        d16[0, :4] = (0, 20000, 19999, 65535)  # dropped, dropped (== 20), kept, dropped
        Image.fromarray(d16).save(os.path.join(base, "depth", f"{fid}.png"))
        Image.fromarray(rgb[k]).save(os.path.join(base, "color", f"{fid}.jpg"), format="PNG")  # lossless under the .jpg name
        np.savetxt(os.path.join(base, "pose", f"{fid}.txt"), T[k])


def main():
    mod = _import_reference()
    with tempfile.TemporaryDirectory() as base:
        make_scene(base)
        pcd = mod.create_downsampled_point_cloud(base, image_size=(W, H), stride=STRIDE, depth_trunc=VOXEL,
                                                 buffer_size=BUFFER, depth_scale=1)  # depth_scale: ignored by get_depth
        names = sorted(os.listdir(os.path.join(base, "depth")))
        ids = [n.split(".")[0] for n in names]
        d16 = np.stack([_pil_read(os.path.join(base, "depth", f"{i}.png")) for i in ids]).astype(np.uint16)
        col = np.stack([_pil_read(os.path.join(base, "color", f"{i}.jpg")) for i in ids]).astype(np.uint8)
        poses = np.stack([np.loadtxt(os.path.join(base, "pose", f"{i}.txt")) for i in ids])
        intr = np.loadtxt(os.path.join(base, "intrinsic", "intrinsic_depth.txt"))
    out = os.path.join(HERE, "scene_cloud_golden.npz")
    np.savez_compressed(out, names=np.array(names), depth_u16=d16, rgb=col, poses=poses, intrinsic=intr,
                        stride=STRIDE, buffer_size=BUFFER, voxel_size=VOXEL, depth_scale=1000,
                        points=np.asarray(pcd.points), colors=np.asarray(pcd.colors))
    print(out, d16.shape, np.asarray(pcd.points).shape, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
