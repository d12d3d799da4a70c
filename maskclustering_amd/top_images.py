"""Projected boxes of the objects' top views on the device (the geometry of ``get_top_images.py``).

The reference's last TASMap stage takes, per final object, the first nine entries of its
``mask_list`` (sorted by coverage by ``find_represent_mask``), projects the object's points into
each of those masks' frames (``get_bbox_by_projection``, :180-237), and draws the pixel bounding box
(``draw_red_bbox``, :241-282).  Here the projection and the box are one C-ABI call
(``mc_proj_boxes``) for all requests of a scene; drawing, the PNG files and the matplotlib grid stay
the reference's.

Run from the reference's root instead of ``python get_top_images.py ...``:

    python -m maskclustering_amd.top_images --config tasmap ...

which imports the reference's module, routes its ``get_bbox_by_projection`` here and runs its
``main``.
"""
from __future__ import annotations

import numpy as np

from . import _device, _native


def _intrinsics_size(intrinsic_cam_parameters):
    """(fx, fy, cx, cy), width, height as the reference reads them (:194-199): from the matrix and the
    intrinsics object's own size, not from the image file"""
    m = np.asarray(intrinsic_cam_parameters.intrinsic_matrix, np.float64)
    return (np.array([m[0, 0], m[1, 1], m[0, 2], m[1, 2]], np.float64), int(intrinsic_cam_parameters.width),
            int(intrinsic_cam_parameters.height))


def get_bbox_by_projection(pcd, intrinsic_cam_parameters, extrinsics):
    """get_top_images.py:180-237 with the reference's signature: pcd with ``.points`` [N, 3],
    an intrinsics object (``intrinsic_matrix``, ``width``, ``height``) and the camera -> world
    matrix.  Returns (px_min, py_min, px_max, py_max) or None."""
    k, width, height = _intrinsics_size(intrinsic_cam_parameters)
    points = np.asarray(pcd.points, np.float64).reshape(-1, 3)
    world_to_cam = np.linalg.inv(extrinsics)                              # :205, LAPACK's as in the reference
    n = len(points)
    boxes, status, _ = _device.context().proj_boxes(points, np.array([0, n], np.int64), np.arange(n, dtype=np.int32),
                                                    k[None], np.asarray(world_to_cam, np.float64)[None], width, height,
                                                    [0], [0])
    if status[0] != _native.MC_PROJ_OK:
        return None
    return tuple(int(v) for v in boxes[0])


def _of_frame(table, frame_id):
    return table(frame_id) if callable(table) else table[frame_id]


def object_boxes(object_dict, scene_points, intrinsics, extrinsics, width, height, top_k=9):
    """Every object's requests in one call, in the reference's order (main(), :393-409): object by
    object in the dictionary's order, then ``value['mask_list'][:top_k]``, objects with an empty list
    skipped.  object_dict as ``utils/post_process.py`` exports it (``point_ids``, ``mask_list`` of
    (frame_id, mask_id, coverage)); scene_points [P, 3]; intrinsics / extrinsics: per frame id (a
    mapping, a sequence or a callable) (fx, fy, cx, cy) or a 3 x 3 matrix, and the camera -> world
    matrix; one image size for all frames.  Returns a list of (key, frame_id, bbox or None)."""
    keys, frames, off, ids = [], [], [0], []
    slot_of, req_obj = {}, []
    for key, value in object_dict.items():
        mask_list = value['mask_list'][:top_k]
        if len(mask_list) == 0:
            continue
        slot_of[key] = len(off) - 1
        pts = np.asarray(list(value['point_ids']), np.int64).reshape(-1)
        ids.append(pts)
        off.append(off[-1] + len(pts))
        for mask_info in mask_list:
            keys.append(key)
            frames.append(mask_info[0])
            req_obj.append(slot_of[key])
    if not keys:
        return []
    distinct = list(dict.fromkeys(frames))
    row = {f: i for i, f in enumerate(distinct)}
    k = np.stack([_device.intrinsics_tuple(_of_frame(intrinsics, f)) for f in distinct])
    w2c = np.stack([np.linalg.inv(np.asarray(_of_frame(extrinsics, f), np.float64)) for f in distinct])
    boxes, status, _ = _device.context().proj_boxes(np.asarray(scene_points, np.float64).reshape(-1, 3),
                                                    np.asarray(off, np.int64), np.concatenate(ids).astype(np.int32), k, w2c,
                                                    int(width), int(height), req_obj, [row[f] for f in frames])
    return [(key, f, tuple(int(v) for v in b) if s == _native.MC_PROJ_OK else None)
            for key, f, b, s in zip(keys, frames, boxes, status)]


def clip_draw_box(bbox, width, height, thickness=2):
    """draw_red_bbox's integer clamp (:262-272): the two corner points it passes to cv2.rectangle,
    each coordinate moved into [margin, side - 1 - margin] with margin = thickness // 2."""
    margin = thickness // 2
    x_min, y_min, x_max, y_max = (int(v) for v in bbox)
    x_min = max(margin, min(x_min, width - 1 - margin))
    y_min = max(margin, min(y_min, height - 1 - margin))
    x_max = max(margin, min(x_max, width - 1 - margin))
    y_max = max(margin, min(y_max, height - 1 - margin))
    return (x_min, y_min), (x_max, y_max)


def main():
    import importlib
    ref = importlib.import_module("get_top_images")           # the reference's, from its root
    ref.get_bbox_by_projection = get_bbox_by_projection
    ref.main()


if __name__ == "__main__":
    main()
