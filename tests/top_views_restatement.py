"""Numpy restatement of the projected boxes (get_top_images.py:193-237, get_bbox_by_projection), of
the selection of an object's top views (value['mask_list'][:9] after find_represent_mask's in-place
sort, utils/post_process.py:126-128) and of draw_red_bbox's clamp (:262-272).  Plain numpy, written
for clarity; it is the CPU statement the device path (mc_proj_*) and
maskclustering_amd/csrc/mc_proj_plan.hpp are compared with, and is itself compared with the
reference's fixtures (tests/test_top_views_cpu.py).

The one freedom the reference leaves is the rounding order of the 4-term dot products of
``world_to_cam @ points_hom.T`` (OpenBLAS dgemm's).  Here, as on the device, each camera coordinate
is ((r0*x + r1*y) + r2*z) + t with every product and sum rounded on its own.  ``project`` also
returns a FRAGILE flag: True when some point lies so close to a decision (z > 0, or a pixel
boundary) that another summation order could decide differently.
"""
from __future__ import annotations

import numpy as np

OK, BEHIND, OUTSIDE = 0, 1, 2
U = 2.0 ** -53                       # unit roundoff of float64
GAMMA4 = 4 * U / (1 - 4 * U)         # Higham's gamma_4: any order of a 4-term dot product is within gamma_4 * sum|a_k b_k|


def camera_coords(points, world_to_cam):
    """(xc, yc, zc, ex, ey, ez): the camera coordinates in the fixed order and the gamma_4 bound of each"""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    m = np.asarray(world_to_cam, np.float64).reshape(4, 4)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    out, err = [], []
    with np.errstate(all="ignore"):
        for r in range(3):
            a, b, c = m[r, 0] * x, m[r, 1] * y, m[r, 2] * z
            out.append(((a + b) + c) + m[r, 3])
            err.append(GAMMA4 * (np.abs(a) + np.abs(b) + np.abs(c) + abs(m[r, 3])))
    return (*out, *err)


def project(points, world_to_cam, intrinsics, width, height):
    """One request: (status, box = (min px, min py, max px, max py) as ints, or (0, 0, 0, 0) without
    one, number of in-bounds points, fragile)."""
    fx, fy, cx, cy = (float(v) for v in np.asarray(intrinsics, np.float64).reshape(4))
    xc, yc, zc, ex, ey, ez = camera_coords(points, world_to_cam)
    with np.errstate(all="ignore"):
        fragile = bool(np.any(np.abs(zc) <= ez))                       # z could change sign
        front = zc > 0                                                 # a NaN z is not > 0
        if not front.any():
            return BEHIND, (0, 0, 0, 0), 0, fragile
        xc, yc, zc, ex, ey, ez = (a[front] for a in (xc, yc, zc, ex, ey, ez))
        qx, qy = xc / zc, yc / zc
        sx, sy = fx * qx, fy * qy
        u, v = sx + cx, sy + cy                                        # three rounded operations each
        ru, rv = np.rint(u), np.rint(v)                                # round half to even, as np.round
        inb = (ru >= 0) & (ru < width) & (rv >= 0) & (rv < height)    # in floating point: -0.0 is in, NaN / inf out
        # how far u, v can move: the coordinates' bounds through the division (first order, z kept
        # away from 0 by its own bound), plus the three operations' own roundings on moved inputs
        zlo = np.maximum(np.abs(zc) - ez, np.finfo(np.float64).tiny)
        du = abs(fx) * (ex + np.abs(qx) * ez) / zlo * (1 + 8 * U) + 4 * U * (np.abs(sx) + abs(cx) + np.abs(u))
        dv = abs(fy) * (ey + np.abs(qy) * ez) / zlo * (1 + 8 * U) + 4 * U * (np.abs(sy) + abs(cy) + np.abs(v))
        # only a point that is, or could become, in bounds on that axis can change the box
        near_u = (u >= -0.5 - du) & (u <= width - 0.5 + du) & (v >= -0.5 - dv) & (v <= height - 0.5 + dv)
        half_u = np.abs(u - (np.floor(u) + 0.5)) <= du
        half_v = np.abs(v - (np.floor(v) + 0.5)) <= dv
        fragile = fragile or bool(np.any(near_u & (half_u | half_v)))
        fragile = fragile or bool(np.any(~np.isfinite(du) & np.isfinite(u)) or np.any(~np.isfinite(dv) & np.isfinite(v)))
    if not inb.any():
        return OUTSIDE, (0, 0, 0, 0), 0, fragile
    px, py = ru[inb].astype(np.int64), rv[inb].astype(np.int64)
    return OK, (int(px.min()), int(py.min()), int(px.max()), int(py.max())), int(inb.sum()), fragile


def boxes(points, obj_pt_off, obj_pts, intrinsics, world_to_cam, width, height, req_object, req_frame):
    """All requests: (boxes int32 [n, 4], status int32 [n], inside int32 [n], fragile bool [n])."""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    n = len(req_object)
    bx, st, ins, fr = np.zeros((n, 4), np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, bool)
    for j, (o, f) in enumerate(zip(req_object, req_frame)):
        ids = np.asarray(obj_pts[obj_pt_off[o]:obj_pt_off[o + 1]], np.int64)
        st[j], bx[j], ins[j], fr[j] = project(points[ids], world_to_cam[f], intrinsics[f], width, height)
    return bx, st, ins, fr


def top_k(coverage, k):
    """positions of the first k entries of a mask list after ``sorted(key=coverage, reverse=True)``:
    descending, equal coverages in list order (both of Python's sorts are stable, and reverse=True
    keeps the order of equal elements)"""
    cov = np.asarray(coverage, np.float64)
    return np.argsort(-cov, kind="stable")[:k]


def top_requests(obj_mask_off, obj_mask_cov, obj_mask_frame, k):
    """(top_pos, top_frame) int32 [num_objects, k], padded with -1"""
    nf = len(obj_mask_off) - 1
    pos, frame = np.full((nf, k), -1, np.int32), np.full((nf, k), -1, np.int32)
    for f in range(nf):
        a, b = int(obj_mask_off[f]), int(obj_mask_off[f + 1])
        t = top_k(obj_mask_cov[a:b], k)
        pos[f, :len(t)] = t
        frame[f, :len(t)] = np.asarray(obj_mask_frame[a:b])[t]
    return pos, frame


def draw_clamp(bbox, width, height, thickness=2):
    """the two corners draw_red_bbox hands to cv2.rectangle"""
    margin = thickness // 2
    x_min, y_min, x_max, y_max = (int(v) for v in bbox)
    x_min = max(margin, min(x_min, width - 1 - margin))
    y_min = max(margin, min(y_min, height - 1 - margin))
    x_max = max(margin, min(x_max, width - 1 - margin))
    y_max = max(margin, min(y_max, height - 1 - margin))
    return (x_min, y_min), (x_max, y_max)
