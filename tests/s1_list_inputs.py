"""Inputs of the S1 eps-list boundary tests (test_gpu_s1_lists.py) and the conditions they must meet,
checked without a GPU (test_s1_list_inputs_cpu.py): a numpy restatement of the oracle's voxel points (the
denoise's inputs; its per-slot voxel counts must equal the oracle's nvox column) gives every point's
eps-neighbour count by brute force.  The restatement's per-voxel sums may differ from the oracle's in the last
bits, so a count can differ by a neighbour that sits exactly on eps: the conditions ask for non-empty
buckets, not for exact sizes."""
import os

import numpy as np

from conftest import GOLDEN

NBCAPS = [7, 8, 9, 16, 17, 64]
MIN_CLASSES = [0, 2, 4, 5, 6]
CLASS_N = [512, 1024, 2048, 3072, 4096, 16384]  # mc::kBpClassN (mc_bp_denoise_lds.inl): the LDS classes' capacities


def dense_inputs():
    """(scene, depth, seg, intrinsics, poses) of the two dense inputs, and of one 1440x1920 frame of the same
    generator: the dense inputs' largest slot has 1198 voxels, so no slot of theirs takes the 3072 class
    (the other classes above 1024 are reached by MC_BP_MIN_CLASS)"""
    from maskclustering_amd.synthetic_frames import make_frames_shape
    z = dict(np.load(os.path.join(GOLDEN, "s1_dense.npz")))
    fr = make_frames_shape("tiny", seed=5, H=360, W=480, num_frames=3)
    big = make_frames_shape("tiny", seed=5, H=1440, W=1920, num_frames=1)  # a slot of 2049 .. 3072 voxels
    return {"s1_dense": (z["in_scene"], z["in_depth"], z["in_seg"], z["in_intrinsics"], z["in_poses"]),
            "tiny": (fr.scene_points, fr.depth, fr.seg, fr.intrinsics, fr.poses),
            "tiny_1440": (big.scene_points, big.depth, big.seg, big.intrinsics, big.poses)}


def oracle_references(inputs):
    """per input: the oracle's (labels, off, pts, stats) of every frame, read-only"""
    from oracle import oracle
    ref = {}
    for name, (scene, depth, seg, K, T) in inputs.items():
        sc = np.asarray(scene, np.float64).astype(np.float32)
        ref[name] = oracle.s1_frames(sc, list(depth), list(seg), K, T)
    for frames in ref.values():
        for out in frames:
            for a in out:
                a.setflags(write=False)
    return ref


def voxel_points(depth, seg, K, T, depth_trunc=20.0, voxel=0.01, few_points=25):
    """the denoise's inputs of one frame, restated in numpy from oracle/s1_oracle.c (world_point,
    voxel_down): {mask id: voxel means [nv, 3] f64, first-occurrence order}"""
    depth = np.asarray(depth, np.float32)
    K = np.asarray(K, np.float64).reshape(4)
    T = np.asarray(T, np.float64).reshape(4, 4)
    out = {}
    for i in np.unique(seg):
        if i == 0:
            continue
        v, u = np.nonzero((seg == i) & (depth > 0) & (depth.astype(np.float64) < depth_trunc))  # row-major
        if len(v) < few_points:
            continue
        z = depth[v, u].astype(np.float64)
        x = (u.astype(np.float64) - K[2]) * z / K[0]
        y = (v.astype(np.float64) - K[3]) * z / K[1]
        r = [((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(4)]
        p = np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1)
        ix = np.floor((p - (p.min(axis=0) - voxel * 0.5)) / voxel).astype(np.int64)
        key = (ix[:, 0] << 42) | (ix[:, 1] << 21) | ix[:, 2]
        _, first, inv = np.unique(key, return_index=True, return_inverse=True)
        rank = np.argsort(np.argsort(first))[inv]  # voxel number in order of first occurrence
        s = np.zeros((len(first), 3))
        np.add.at(s, rank, p)  # sequential in input order, as the oracle's sums
        out[int(i)] = s / np.bincount(rank)[:, None]
    return out


def eps_counts(p, eps=0.04):
    """points within eps of each point (self included), the kernels' and the oracle's f64 expression"""
    cnt = np.zeros(len(p), np.int64)
    for a in range(0, len(p), 512):
        d = p[a:a + 512, None, :] - p[None, :, :]
        d2 = ((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])
        cnt[a:a + 512] = (d2 < eps * eps).sum(axis=1)
    return cnt


def input_profile(inputs, references):
    """(eps-neighbour counts of every voxel point, voxel counts of every slot) over the inputs"""
    counts, nvox = [], []
    for name, (_, depth, seg, K, T) in inputs.items():
        for f in range(len(depth)):
            vp = voxel_points(depth[f], seg[f], K[f], T[f])
            st = references[name][f][3]
            want = {int(r[0]): int(r[2]) for r in st if r[1] >= 25}
            assert {i: len(p) for i, p in vp.items()} == want, f"{name} frame {f}: voxel counts differ from the oracle's"
            for p in vp.values():
                counts.append(eps_counts(p))
                nvox.append(len(p))
    return np.concatenate(counts), np.asarray(nvox)


def check_inputs_reach_every_boundary_and_class(inputs, references):
    """the conditions on the inputs, from the inputs and the oracle alone; returns the histogram and the classes"""
    counts, nvox = input_profile(inputs, references)
    hist = np.bincount(counts, minlength=66)
    for c in (8, 16, 24, 32, 40, 48, 56):
        assert hist[c] > 0, f"no point with {c} eps-neighbours (a full last word)"
    assert hist[64] > 0, "no point with exactly 64 eps-neighbours (the cap)"
    assert hist[65:].sum() > 0, "no point with more than 64 eps-neighbours (entries past the cap)"
    for c in NBCAPS:  # each cap has lists on both of its sides
        assert hist[1:c + 1].sum() > 0 and hist[c + 1:].sum() > 0, c
    # the class a slot of n voxels lands in under MC_BP_MIN_CLASS = m: max(m, its class by size) (k_bp_classify)
    by_size = np.searchsorted(np.asarray(CLASS_N), nvox, side="left")
    reached = {int(max(m, c)) for m in MIN_CLASSES for c in by_size}
    for c, n in enumerate(CLASS_N):
        assert c in reached, f"no slot lands in the {n} class under any MC_BP_MIN_CLASS of the cases"
    assert len(CLASS_N) in reached  # and the global-memory kernel
    return hist, sorted(reached)
