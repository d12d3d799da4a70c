"""Restatement of the scene point cloud fusion (tasmap/tasmap2mct_format.py:216-284: backproject,
create_downsampled_point_cloud) in numpy, independent of the kernels: the witness of
tests/test_scene_cloud_cpu.py and tests/test_gpu_scene_cloud.py.

* world points elementwise in float64 in the stated order: z = (double)d, x = ((u - cx) z) / fx,
  y = ((v - cy) z) / fy, each pose row as ((T0 x + T1 y) + T2 z) + T3, then the divide by row 3 (numpy
  rounds every elementwise operation on its own; no BLAS product, no long double);
* voxel_down_sample: vmin = min - voxel / 2, index = floor((p - vmin) / voxel), voxels numbered by first
  occurrence, sums by np.add.at (unbuffered and in index order: the left fold), mean = sum / count;
* the buffer schedule written from the reference's loop (:271-282)."""
import numpy as np

DEPTH_LIMIT = 20.0


def valid_pixels(depth, depth_trunc=DEPTH_LIMIT):
    """bool [H, W]: 0 < d < depth_trunc (Open3D zeroes d >= depth_trunc, then drops d <= 0; NaN fails both)."""
    d = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        return (d > 0) & (d.astype(np.float64) < float(depth_trunc))


def frame_points(depth, rgb, K, T, depth_trunc=DEPTH_LIMIT):
    """(points f64 [n, 3], colours f64 [n, 3]) of one frame's valid pixels, row-major."""
    depth = np.asarray(depth, np.float32)
    K = np.asarray(K, np.float64).reshape(4)
    T = np.asarray(T, np.float64).reshape(4, 4)
    v, u = np.nonzero(valid_pixels(depth, depth_trunc))  # row-major order
    z = depth[v, u].astype(np.float64)
    x = ((u.astype(np.float64) - K[2]) * z) / K[0]
    y = ((v.astype(np.float64) - K[3]) * z) / K[1]
    r = [((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(4)]
    pts = np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1)
    col = np.asarray(rgb, np.uint8)[v, u].astype(np.float64) / 255.0
    return pts.reshape(-1, 3), col.reshape(-1, 3)


def voxel_numbers(points, voxel):
    """(voxel number of every point, number of voxels): voxels numbered by first occurrence."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    if len(p) == 0:
        return np.zeros(0, np.int64), 0
    vmin = p.min(axis=0) - voxel * 0.5
    ix = np.floor((p - vmin) / voxel).astype(np.int64)
    if ix.max() < (1 << 21):  # one packed key a point: the same grouping, a 1-D sort
        _, first, inv = np.unique((ix[:, 0] << 42) | (ix[:, 1] << 21) | ix[:, 2], return_index=True, return_inverse=True)
    else:
        _, first, inv = np.unique(ix, axis=0, return_index=True, return_inverse=True)
    inv = np.asarray(inv).reshape(-1)
    order = np.argsort(first, kind="stable")  # unique row -> rank of its first occurrence
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank[inv], len(order)


def voxel_down_sample(points, colors, voxel):
    """(means f64 [nv, 3], colour means or None, populations int64 [nv])."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    vid, nv = voxel_numbers(p, voxel)
    cnt = np.bincount(vid, minlength=nv).astype(np.int64)
    s = np.zeros((nv, 3), np.float64)
    np.add.at(s, vid, p)
    means = s / cnt[:, None].astype(np.float64) if nv else s
    cm = None
    if colors is not None:
        c = np.asarray(colors, np.float64).reshape(-1, 3)
        sc = np.zeros((nv, 3), np.float64)
        np.add.at(sc, vid, c)
        cm = sc / cnt[:, None].astype(np.float64) if nv else sc
    return means, cm, cnt


def flush_schedule(F, B):
    """[(first frame, end frame)] of the flushed buffers: the reference's loop."""
    out, buf = [], []
    for i in range(F):
        buf.append(i)
        if (i + 1) % B == 0:
            out.append((buf[0], buf[-1] + 1))
            buf = []
    if buf:
        out.append((buf[0], buf[-1] + 1))
    return out


def fuse_frames(depth, rgb, intrinsics, poses, voxel_size=0.005, buffer_size=10, depth_trunc=DEPTH_LIMIT, info=None):
    """(points, colours) of create_downsampled_point_cloud on decoded frames; info (a dict) receives the
    populations of every voxel_down_sample run and the run's input size."""
    F = len(depth)
    full_p, full_c, pops, sizes = [np.zeros((0, 3))], [np.zeros((0, 3))], [], []
    for f0, f1 in flush_schedule(F, buffer_size):
        fp = [frame_points(depth[f], rgb[f], intrinsics[f], poses[f], depth_trunc) for f in range(f0, f1)]
        p = np.concatenate([a for a, _ in fp])
        c = np.concatenate([b for _, b in fp])
        mp, mc, cnt = voxel_down_sample(p, c, voxel_size)
        full_p.append(mp), full_c.append(mc), pops.append(cnt), sizes.append(len(p))
    p, c = np.concatenate(full_p), np.concatenate(full_c)
    mp, mc, cnt = voxel_down_sample(p, c, voxel_size)
    pops.append(cnt), sizes.append(len(p))
    if info is not None:
        info["populations"] = pops
        info["sizes"] = sizes
    return mp, mc


def synthetic_frames(F=7, H=48, W=64, seed=0, general_pose_frame=None, focal=60.0):
    """A small RGB-D capture: a camera moving past a tilted wall with a box in front, depths 0.6-3 m, some
    holes; rigid poses, and (general_pose_frame) one frame whose pose row 3 is not (0, 0, 0, 1)."""
    rng = np.random.default_rng(seed)
    depth = np.zeros((F, H, W), np.float32)
    rgb = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    K = np.zeros((F, 4))
    T = np.zeros((F, 4, 4))
    vv, uu = np.mgrid[0:H, 0:W]
    for f in range(F):
        K[f] = (focal + 0.25 * f, focal + 1.0, W / 2 - 0.5 + 0.125 * f, H / 2 - 0.5)
        d = 2.0 + 0.64 / W * uu + 0.192 / H * vv + 0.05 * f + 0.002 * rng.standard_normal((H, W))
        box = (uu > W // 3) & (uu < W // 2) & (vv > H // 4) & (vv < 3 * H // 4)
        d = np.where(box, 0.6 + 0.048 / H * vv, d)
        d[rng.random((H, W)) < 0.05] = 0.0
        depth[f] = d.astype(np.float32)
        a = 0.05 * f
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        T[f] = np.eye(4)
        T[f, :3, :3] = R
        T[f, :3, 3] = (0.1 * f, -0.02 * f, 0.03 * f)
    if general_pose_frame is not None:
        T[general_pose_frame, 3] = (0.001, -0.002, 0.0005, 1.25)
    return depth, rgb, K, T
