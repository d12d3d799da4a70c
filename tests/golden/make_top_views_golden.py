"""Golden fixture for the projected boxes (mc_proj_*): the REFERENCE's own ``get_top_images.py``
run on synthetic objects and cameras, its outputs captured.

Run ONLY in the build container, where /root/reference exists:

    python tests/golden/make_top_views_golden.py

The reference module is loaded from its file, unmodified, with stand-ins for what this container
lacks or what it must not touch: ``cv2`` (``rectangle`` records its arguments, which is how
draw_red_bbox's clamp is captured), ``open3d``, ``matplotlib.pyplot``, ``tqdm`` and ``utils.config``.
``get_bbox_by_projection`` is given ``pcd`` as an object with ``.points`` and the intrinsics as an
object with ``intrinsic_matrix``, ``width`` and ``height``.

Stored in top_views.npz (data only):
  scene set   about 3000 points, eight objects, six cameras with random rigid poses aimed at the
              scene, at 131 x 97 and at 640 x 480; every (object, frame) once plus duplicates, in a
              shuffled order.  Objects: wholly visible ones, ones cut by the image edge, one behind
              the camera in some frames, one in front but outside, a single point, an empty one and
              one of more than 1000 points.  Status 0 = a box, 1 = None at :215-216 (nothing in
              front), 2 = None at :228-229 (nothing in the image); which of the two Nones it was is
              read from the reference's own z_cam > 0 test, redone here on its own matrix product.
  edge set    identity pose and one axis-permuting pose with +-1 entries (the dot product is exact
              in any order), fx = fy = 2, cx = cy = 0, single points at the rounding edges listed in
              edge_cases(), z in {0, -1, 1e-320}, an all -inf extrinsic, the empty object
  clamp set   draw_red_bbox's cv2.rectangle corners for thickness 2 and 5
The maker asserts that at most 1 % of the scene requests are FRAGILE (top_views_restatement.py) and
that the restatement equals the reference on every other request and on the whole edge set.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import top_views_restatement as R  # noqa: E402

REF = "/root/reference"
RECT = []          # the cv2.rectangle stand-in's calls


def _install_stubs():
    cv2 = types.ModuleType("cv2")
    cv2.INTER_NEAREST = 0

    def rectangle(img, p0, p1, color, thickness):
        RECT.append((tuple(int(v) for v in p0), tuple(int(v) for v in p1), tuple(color), int(thickness)))

    cv2.rectangle = rectangle
    o3d = types.ModuleType("open3d")
    mpl = types.ModuleType("matplotlib")
    plt = types.ModuleType("matplotlib.pyplot")
    mpl.pyplot = plt
    tqdm = types.ModuleType("tqdm")
    tqdm.tqdm = lambda it, **k: it
    utils = types.ModuleType("utils")
    cfg = types.ModuleType("utils.config")
    cfg.get_args = lambda: SimpleNamespace()
    cfg.get_dataset = lambda a: SimpleNamespace()
    utils.config = cfg
    sys.modules.update({"cv2": cv2, "open3d": o3d, "matplotlib": mpl, "matplotlib.pyplot": plt, "tqdm": tqdm,
                        "utils": utils, "utils.config": cfg})


def _load_reference():
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("ref_get_top_images", os.path.join(REF, "get_top_images.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _intr(k, width, height):
    m = np.array([[k[0], 0, k[2]], [0, k[1], k[3]], [0, 0, 1]], np.float64)
    return SimpleNamespace(intrinsic_matrix=m, width=int(width), height=int(height))


def _ask(mod, points, k, width, height, ext):
    """(status, box) of the reference for one request"""
    points = np.asarray(points, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        got = mod.get_bbox_by_projection(SimpleNamespace(points=points), _intr(k, width, height), ext)
        if got is not None:
            assert len(got) == 4
            return R.OK, [int(v) for v in got]
        # which None: the reference's own product and test (:205-212), redone
        hom = np.hstack([points, np.ones((len(points), 1), dtype=np.float32)])
        z = (np.linalg.inv(ext) @ hom.T).T[:, 2]
        return (R.OUTSIDE if np.any(z > 0) else R.BEHIND), [0, 0, 0, 0]


def _look_at(eye, target, roll):
    """camera -> world: x right, y down, z forward"""
    fwd = target - eye
    fwd /= np.linalg.norm(fwd)
    up = np.array([0.0, 0.0, 1.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    c, s = np.cos(roll), np.sin(roll)
    right, down = c * right + s * down, -s * right + c * down
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = right, down, fwd, eye
    return m


def make_scene(rng):
    F = 6
    az = rng.uniform(0, 2 * np.pi, F)
    az[0] = 0.0
    eyes = np.stack([4.0 * np.cos(az), 4.0 * np.sin(az), rng.uniform(-0.5, 1.0, F)], 1)
    eyes[0, 2] = 0.0
    ext = np.stack([_look_at(eyes[f], rng.normal(0, 0.3, 3), rng.uniform(-0.4, 0.4)) for f in range(F)])
    blob = lambda c, s, n: np.asarray(c, np.float64) + rng.normal(0, 1, (n, 3)) * np.asarray(s, np.float64)  # noqa: E731
    parts = [blob((0.0, 0.0, 0.0), 0.25, 400),          # 0: small, central: wholly visible
             blob((0.5, 1.5, 0.2), (1.2, 1.2, 0.9), 500),  # 1: wide: cut by the image edge
             blob((-0.5, -0.5, 0.0), 0.8, 1200),          # 2: more than 1000 points
             blob((0.3, -0.2, 0.4), 0.0, 1),              # 3: a single point
             np.zeros((0, 3)),                            # 4: empty
             blob((7.0, 0.0, 0.0), 0.2, 150),             # 5: behind camera 0 (which sits at x = 4 looking at the origin)
             blob((0.0, 0.0, 30.0), 0.2, 150),            # 6: high above: in front of the cameras but outside
             blob((-1.5, 1.0, -0.8), (0.9, 0.5, 0.7), 600)]  # 7: another one cut by the edge
    pts = np.concatenate(parts)
    perm = rng.permutation(len(pts))                      # the objects' ids are not contiguous runs
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(pts))
    points = pts[perm]
    off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    ids = inv.astype(np.int32)                            # object o's points: ids[off[o]:off[o + 1]]
    sizes = np.array([[131, 97], [640, 480]], np.int32)
    intr = np.array([[[100.0, 100.0, 65.0, 48.0]] * F, [[500.0, 505.0, 320.5, 239.5]] * F])
    req = [(o, f) for o in range(len(parts)) for f in range(F)]
    req += [req[i] for i in rng.integers(0, len(req), 6)]  # duplicates
    req = np.array(req, np.int32)[rng.permutation(len(req))]
    return points, off, ids, ext, sizes, intr, req


PERM = np.array([[0.0, -1.0, 0.0, 0.0],    # world -> camera with +-1 entries: xc = -yw, yc = zw, zc = -xw
                 [0.0, 0.0, 1.0, 0.0],
                 [-1.0, 0.0, 0.0, 0.0],
                 [0.0, 0.0, 0.0, 1.0]])
EDGE_VALUES = (-0.26, -0.25, 0.25, 0.75, 1.25, 65.25, 319.75)
EDGE_SIDES = (131, 640, 8)


def edge_cases():
    """(name, camera points [k, 3], world_to_cam, width, height) with fx = fy = 2, cx = cy = 0"""
    cases = []
    for pname, w2c in (("id", np.eye(4)), ("perm", PERM)):
        for a in EDGE_VALUES:
            for side in EDGE_SIDES:
                cases.append((f"{pname} x={a} w={side}", [(a, 0.25, 1.0)], w2c, side, 97))
                cases.append((f"{pname} y={a} h={side}", [(0.25, a, 1.0)], w2c, 97, side))
        for z in (0.0, -1.0, 1e-320):
            cases.append((f"{pname} z={z}", [(0.0, 0.0, z)], w2c, 131, 97))
        cases.append((f"{pname} z=1e-320 x=1", [(1.0, 0.0, 1e-320)], w2c, 131, 97))
        cases.append((f"{pname} empty", [], w2c, 131, 97))
        cases.append((f"{pname} two points", [(0.25, 0.75, 1.0), (1.25, -0.25, 1.0), (5.0, 5.0, -1.0)], w2c, 131, 97))
    cases.append(("all -inf", [(0.25, 0.25, 1.0)], None, 131, 97))
    return cases


def run_edges(mod):
    k = np.array([2.0, 2.0, 0.0, 0.0])
    out = dict(name=[], pts=[], npts=[], ext=[], size=[], status=[], box=[])
    for name, cam, w2c, width, height in edge_cases():
        cam = np.asarray(cam, np.float64).reshape(-1, 3)
        if w2c is None:
            ext = np.full((4, 4), -np.inf)
            world = cam
        else:
            ext = w2c.T.copy()                            # a signed permutation: its inverse, exactly
            assert np.array_equal(np.linalg.inv(ext), w2c), "LAPACK inverts a signed permutation exactly"
            world = cam @ ext[:3, :3].T                    # exact: one +-1 term per coordinate
        st, box = _ask(mod, world, k, width, height, ext)
        padded = np.zeros((3, 3))
        padded[:len(world)] = world
        for key, v in zip(out, (name, padded, len(world), ext, (width, height), st, box)):
            out[key].append(v)
        print(f"  {name:28s} -> status {st} box {box}")
    return {f"edge_{k_}": np.array(v) for k_, v in out.items()}, k


CLAMP_CASES = [((0, 0, 130, 96), 131, 97), ((20, 30, 60, 70), 131, 97), ((200, 150, 300, 160), 131, 97),
               ((-50, -40, -10, -5), 131, 97), ((90, 50, 10, 5), 131, 97), ((0, 0, 639, 479), 640, 480), ((0, 0, 2, 2), 3, 3)]


def run_clamps(mod):
    rows = []
    for thickness in (2, 5):
        for bbox, width, height in CLAMP_CASES:
            RECT.clear()
            mod.draw_red_bbox(np.zeros((height, width, 3), np.uint8), bbox, thickness)
            assert len(RECT) == 1 and RECT[0][3] == thickness
            rows.append([*bbox, width, height, thickness, *RECT[0][0], *RECT[0][1]])
    RECT.clear()
    mod.draw_red_bbox(np.zeros((97, 131, 3), np.uint8), None)
    assert not RECT, "no box, nothing drawn"
    return np.array(rows, np.int32)


def main():
    _install_stubs()
    mod = _load_reference()
    rng = np.random.default_rng(11)
    points, off, ids, ext, sizes, intr, req = make_scene(rng)
    n = len(req)
    status, box = np.zeros((2, n), np.int32), np.zeros((2, n, 4), np.int32)
    fragile = mismatch = 0
    w2c = np.stack([np.linalg.inv(e) for e in ext])
    seen = set()
    for s in range(2):
        W, H = (int(v) for v in sizes[s])
        for j, (o, f) in enumerate(req):
            p = points[ids[off[o]:off[o + 1]]]
            status[s, j], box[s, j] = _ask(mod, p, intr[s, f], W, H, ext[f])
            st, bx, ins, fr = R.project(p, w2c[f], intr[s, f], W, H)
            fragile += fr
            if not fr and (st != status[s, j] or list(bx) != list(box[s, j])):
                mismatch += 1
                print("MISMATCH", s, j, o, f, (st, bx), (status[s, j], box[s, j]))
            if st == R.OK:
                seen.add("whole" if ins == len(p) else "cut")
                seen.add("edge" if (bx[0] == 0 or bx[1] == 0 or bx[2] == W - 1 or bx[3] == H - 1) else "interior")
    print(f"scene set: {2 * n} requests, status counts {np.bincount(status.ravel(), minlength=3)}, fragile {fragile}, "
          f"mismatches {mismatch}")
    assert mismatch == 0
    assert fragile <= 0.01 * 2 * n, "the fragile share of the scene set exceeds 1 %"
    assert set(np.unique(status)) == {0, 1, 2} and seen == {"whole", "cut", "edge", "interior"}, (np.unique(status), seen)
    assert len(points) >= 3000 and (np.diff(off) > 1000).any() and (np.diff(off) == 0).any() and (np.diff(off) == 1).any()
    assert len({tuple(r) for r in req}) < n, "duplicates"
    print("edge set:")
    edges, ek = run_edges(mod)
    for j in range(len(edges["edge_status"])):
        e = edges["edge_ext"][j]
        with np.errstate(all="ignore"):
            st, bx, _, _ = R.project(edges["edge_pts"][j][:edges["edge_npts"][j]], np.linalg.inv(e), ek,
                                     *(int(v) for v in edges["edge_size"][j]))
        assert st == edges["edge_status"][j] and list(bx) == list(edges["edge_box"][j]), (edges["edge_name"][j], st, bx)
    clamps = run_clamps(mod)
    path = os.path.join(HERE, "top_views.npz")
    np.savez_compressed(path, points=points, obj_pt_off=off, obj_pts=ids, extrinsics=ext, sizes=sizes, intrinsics=intr,
                        requests=req, status=status, boxes=box, edge_intrinsics=ek, clamps=clamps, **edges)
    size = os.path.getsize(path)
    assert size < 600_000, size
    print(f"top_views.npz: {size / 1e3:.1f} kB")


if __name__ == "__main__":
    main()
