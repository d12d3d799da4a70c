"""Inputs of the S1 ball-query tests (test_gpu_s1_query.py) and the conditions they must meet, checked without a
GPU (test_s1_query_inputs_cpu.py).  The staged query (k_bp_query_lds) keeps a slot whose float32 box covers at
most MC_BP_QUERY_CELLS cells of the 2r scene grid and holds at most MC_BP_QUERY_CAND scene points, and hands the
rest to k_bp_query: the cases need slots on both sides of each cap, overfull balls, scene points on cell
borders and duplicates.  All of it is asserted from the inputs and the oracle alone:
  * a slot's crop size is the oracle's ncand column;
  * a slot's box is not an oracle output, so its cell count is bounded from both sides: the box lies inside
    the float32 box of the mask's voxel means (the survivors are some of them; s1_list_inputs.voxel_points
    restates them), and a kept mask's neighbour ids lie strictly inside the box.  scene_cell is monotone, so
    the cells of the outer box bound the slot's cells from above and those of the neighbours' box from below.
"""
import functools
import os

import numpy as np

from conftest import GOLDEN
from s1_list_inputs import voxel_points

FEW = 25
CELL_BIAS = 1 << 20
# the caps of the split cases (MC_BP_QUERY_CAND, MC_BP_QUERY_CELLS): chosen from the inputs' own
# distributions (both near the medians: crops of 34 .. 1580 scene points, boxes of 140 .. 12672 cells; no
# slot of these inputs is as small as 64 cells)
SPLIT_CAND = 200
SPLIT_CELLS = 640
DEFAULT_CAND, DEFAULT_CELLS = 1024, 4096  # kBpQcCand, kBpQcCells (mc_bp_query.inl)
# parameter sets under which the first-K rule binds (ball_k below the in-ball count of some point)
FIRSTK = [dict(ball_k=1), dict(ball_k=7), dict(ball_radius=0.03, ball_k=20)]
QUANT = 0.005


def scene_cell(v, inv):
    """mc_bp_qcell.hpp scene_cell on float32 arrays: the float32 product, floor, the clamps, the bias"""
    c = np.floor(np.asarray(v, np.float32) * np.float32(inv)).astype(np.int64)
    return np.clip(c, -CELL_BIAS, CELL_BIAS - 1) + CELL_BIAS


def box_cells(lo, hi, radius=0.01):
    """cells of the float32 box [lo, hi] on the grid of cell width 2 * radius"""
    inv = np.float32(1.0) / (np.float32(2.0) * np.float32(radius))
    n = scene_cell(np.asarray(hi, np.float32), inv) - scene_cell(np.asarray(lo, np.float32), inv) + 1
    return int(n[0]) * int(n[1]) * int(n[2])


@functools.lru_cache(maxsize=1)
def inputs():
    """name -> (scene f32 [P, 3], depth, seg, intrinsics, poses): the committed dense frames, three 480 x 360
    frames of the tiny shape and the small shape at its own 160 x 120 (rendered once, not to be written to)"""
    from maskclustering_amd.synthetic_frames import make_frames_shape
    z = dict(np.load(os.path.join(GOLDEN, "s1_dense.npz")))
    tiny = make_frames_shape("tiny", seed=5, H=360, W=480, num_frames=3)
    small = make_frames_shape("small", seed=0)
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32)  # noqa: E731
    return {"s1_dense": (f32(z["in_scene"]), z["in_depth"], z["in_seg"], z["in_intrinsics"], z["in_poses"]),
            "tiny": (f32(tiny.scene_points), tiny.depth, tiny.seg, tiny.intrinsics, tiny.poses),
            "small": (f32(small.scene_points), small.depth, small.seg, small.intrinsics, small.poses)}


def quantised_input():
    """the tiny frames rendered as they are, over a scene whose coordinates are multiples of 0.005 in float32
    (every fourth multiple is a border of the 0.02 cells; the jittered grid collapses some points onto one)"""
    scene, depth, seg, K, T = inputs()["tiny"]
    q = (np.round(scene.astype(np.float64) / QUANT) * QUANT).astype(np.float32)
    return q, depth, seg, K, T


def clustered_input(stride=16, copies=9, jitter=0.003):
    """the tiny frames over the tiny scene with every 16th point repeated nine times within 3 mm, the copies
    appended (the highest ids): a ball of 1 cm around such a point holds ten scene points, one of 3 cm more
    than twenty, and every crop still fits the staged query's default caps"""
    scene, depth, seg, K, T = inputs()["tiny"]
    rng = np.random.default_rng(7)
    base = np.repeat(scene[::stride], copies, axis=0).astype(np.float64)
    rep = (base + rng.uniform(-jitter, jitter, size=base.shape)).astype(np.float32)
    return np.concatenate([scene, rep]), depth, seg, K, T


def shifted_input(shift=1.0):
    """the tiny frames over the scene moved by `shift` metres in z: no scene point near any mask"""
    scene, depth, seg, K, T = inputs()["tiny"]
    return (scene + np.float32([0.0, 0.0, shift])).astype(np.float32), depth, seg, K, T


def references(inp, **prm):
    """the oracle's (labels, off, pts, stats) of every frame of one input, read-only"""
    from oracle import oracle
    scene, depth, seg, K, T = inp
    ref = oracle.s1_frames(scene, list(depth), list(seg), K, T, oracle.BpParams.default(**prm) if prm else None)
    for out in ref:
        for a in out:
            a.setflags(write=False)
    return ref


def slot_profile(inp, ref, radius=0.01):
    """per slot that reaches the query (nsor >= few): (ncand, lower and upper bound of its box cells); the
    lower bound is 0 for a mask that is not kept"""
    scene, depth, seg, K, T = inp
    rows = []
    for f, (lab, off, pts, st) in enumerate(ref):
        vp = voxel_points(depth[f], seg[f], K[f], T[f])
        kept = {int(i): pts[off[k]:off[k + 1]] for k, i in enumerate(lab)}
        for r in st:
            if r[1] < FEW or r[4] < FEW:
                continue
            p = vp[int(r[0])].astype(np.float32)
            # (one ulp wider: the restated voxel means may differ from the oracle's in the last bits)
            upper = box_cells(np.nextafter(p.min(axis=0), np.float32(-np.inf)),
                              np.nextafter(p.max(axis=0), np.float32(np.inf)), radius)
            nb = kept.get(int(r[0]))
            lower = 0
            if nb is not None and len(nb):
                s = scene[nb]
                lower = box_cells(s.min(axis=0), s.max(axis=0), radius)
            rows.append((int(r[5]), lower, upper))
    return np.asarray(rows, np.int64).reshape(-1, 3)


def check_split(inp, ref, cand_cap=SPLIT_CAND, cell_cap=SPLIT_CELLS):
    """slots on both sides of each cap of the split cases"""
    prof = slot_profile(inp, ref)
    ncand, lower, upper = prof[:, 0], prof[:, 1], prof[:, 2]
    assert (ncand > cand_cap).any() and (ncand <= cand_cap).any(), "no slot on one side of the crop cap"
    assert (lower > cell_cap).any(), "no slot surely above the cell cap"
    assert (upper <= cell_cap).any(), "no slot surely within the cell cap"
    return prof


def check_all_staged(inp, ref, radius=0.01):
    """every slot fits the default caps: the whole input takes the staged kernel"""
    prof = slot_profile(inp, ref, radius)
    assert len(prof) and (prof[:, 0] <= DEFAULT_CAND).all() and (prof[:, 2] <= DEFAULT_CELLS).all()
    return prof


def neighbour_sets(ref):
    """{(frame, id): neighbour ids} of the kept masks"""
    return {(f, int(i)): pts[off[k]:off[k + 1]].tobytes() for f, (lab, off, pts, _) in enumerate(ref)
            for k, i in enumerate(lab)}


def check_first_k_binds(inp, prm):
    """the oracle's neighbour sets under prm differ from those under ball_k = 32 for at least one mask: some
    point has more than ball_k scene points in its ball, and the truncation changes a set"""
    a = neighbour_sets(references(inp, **prm))
    b = neighbour_sets(references(inp, **dict(prm, ball_k=32)))
    assert a != b, f"first-K does not bind under {prm}"
    return a, b


def check_quantised(scene, radius=0.01):
    """scene points within one ulp of a cell border in x, and points that share all three coordinates"""
    inv = np.float32(1.0) / (np.float32(2.0) * np.float32(radius))
    c = scene[:, 0] * inv
    near = np.abs(c - np.round(c)) <= np.spacing(np.abs(c).astype(np.float32))
    assert near.any(), "no scene point within one ulp of a cell border"
    uniq = np.unique(scene, axis=0)
    assert len(uniq) < len(scene), "no scene points that share all three coordinates"
    return int(near.sum()), len(scene) - len(uniq)
