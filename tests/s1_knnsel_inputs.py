"""Inputs of the S1 k-NN selection tests (test_gpu_s1_knnsel.py) and the conditions they must meet, checked
without a GPU (test_s1_knnsel_inputs_cpu.py) from the inputs, the oracle and a numpy restatement of the
distance class (mc_bp_knnsel.hpp: min(15, (unsigned)(d2 * (16 / eps2)))).  Three frames of 160 x 120:

  frame 0  id 1: a fronto-parallel wall at z = 0.75 under fx = fy = 64 and the identity pose: its points are
                 exact multiples of 3 * 2^-8 (wider than a voxel, so every pixel is its own voxel mean), a
                 lattice on which squared distances tie exactly; 35 % of its pixels are left out at random, so
                 the points' neighbourhoods are different subsets of the lattice and their selected sets take
                 many sizes
           id 2: a patch of the same wall and a far, small second component (under 20 % of the voxels), which
                 the class filter drops: the slot's kept flags are read
           id 3: 30 pixels at z = 0.375 that share about a dozen voxels: fewer than 20 kept points in all
  frame 1  id 1: 72 x 50 pixels of the wall, whole, under a translated pose: 3600 voxels, sorted positions up
                 to 3599 (all twelve position bits of an entry)
  frame 2  id 1: a tilted, jittered surface (no ties): the generic case
Edges and corners of the walls have fewer than 20 neighbours (the ring queue)."""
import numpy as np

from s1_list_inputs import voxel_points

H, W = 120, 160
EPS = 0.04
KNN = 20
KNN_NET = 24  # kKnnNet (mc_bp_knnsel.hpp)
MIN_CLASSES = [0, 2, 4, 5, 6]
NBCAPS = [64, 30]  # 30: below the wall's interior count of 37, so most of its lists go to the ring queue


def knnsel_inputs():
    """(scene, depth, seg, intrinsics, poses)"""
    rng = np.random.default_rng(11)
    depth = np.zeros((3, H, W), np.float32)
    seg = np.zeros((3, H, W), np.uint8)
    K = np.tile(np.array([64.0, 64.0, 80.0, 60.0]), (3, 1))
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1, :3, 3] = [0.5, -0.25, 2.0]
    # frame 0
    depth[0] = 0.75
    seg[0, 0:48, 0:64] = np.where(rng.random((48, 64)) < 0.65, 1, 0)
    seg[0, 60:90, 0:40] = 2
    seg[0, 100:110, 100:110] = 2
    depth[0, 100:110, 100:110] = 1.5
    seg[0, 100:105, 0:6] = 3
    depth[0, 100:105, 0:6] = 0.375
    # frame 1
    depth[1] = 0.75
    seg[1, 0:50, 0:72] = 1
    # frame 2
    u = np.arange(W)[None, :]
    v = np.arange(H)[:, None]
    depth[2] = (0.8 + 0.002 * u + 0.001 * v + rng.normal(0.0, 0.002, (H, W))).astype(np.float32)
    seg[2, 20:84, 30:94] = 1
    # the scene: every masked pixel's world point
    pts = []
    for f in range(3):
        vv, uu = np.nonzero(seg[f])
        z = depth[f, vv, uu].astype(np.float64)
        p = np.stack([(uu - K[f, 2]) * z / K[f, 0], (vv - K[f, 3]) * z / K[f, 1], z], axis=1) + T[f, :3, 3]
        pts.append(p)
    return np.concatenate(pts), depth, seg, K, T


def oracle_reference(inp):
    """the oracle's (labels, off, pts, stats) of every frame, read-only"""
    from oracle import oracle
    scene, depth, seg, K, T = inp
    ref = oracle.s1_frames(np.asarray(scene, np.float64).astype(np.float32), list(depth), list(seg), K, T)
    for out in ref:
        for a in out:
            a.setflags(write=False)
    return ref


def knn_class(d2, eps2=EPS * EPS):
    """mc::knn_class on an array of squared distances below eps2"""
    return np.minimum(15, (d2 * (16.0 / eps2)).astype(np.uint32))


def selection_profile(p, idx=None, eps=EPS):
    """per point (of idx, or every point) of a slot whose points are all kept: (eps-neighbour count, self
    included; size of the selected set, 0 where the count is below KNN)"""
    idx = range(len(p)) if idx is None else idx
    cnt = np.zeros(len(idx), np.int64)
    sel = np.zeros(len(idx), np.int64)
    for a, i in enumerate(idx):
        d = p[i] - p
        d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        near = d2[d2 < eps * eps]
        cnt[a] = len(near)
        if len(near) >= KNN:
            cum = np.cumsum(np.bincount(knn_class(near), minlength=16))
            sel[a] = cum[np.argmax(cum >= KNN)]
    return cnt, sel


def check_inputs(inp, ref):
    """the conditions on the inputs, from the inputs and the oracle alone"""
    scene, depth, seg, K, T = inp
    vp = [voxel_points(depth[f], seg[f], K[f], T[f]) for f in range(3)]
    stats = [{int(r[0]): r for r in ref[f][3] if r[1] >= 25} for f in range(3)]
    for f in range(3):  # the restatement's slots are the oracle's
        assert {i: len(p) for i, p in vp[f].items()} == {i: int(r[2]) for i, r in stats[f].items()}, f
    # frame 0 id 1: the lattice wall; every point kept, so a list's kept entries are its entries
    wall = vp[0][1]
    assert int(stats[0][1][3]) == len(wall) and len(wall) <= 4096
    assert np.array_equal(wall / (3.0 * 2.0 ** -8), np.round(wall / (3.0 * 2.0 ** -8)))  # an exact lattice
    cnt, sel = selection_profile(wall)
    assert cnt.max() <= 64  # every list within the cap
    assert (sel > KNN_NET).any(), "no point whose selected set exceeds the network (the leftover path)"
    assert (sel == KNN).any(), "no point whose selected set is exactly k"
    assert (cnt < KNN).any(), "no point with fewer than k list entries (the ring queue)"
    # frame 0 id 2: a component the 20 % filter drops
    assert 0 < int(stats[0][2][3]) < int(stats[0][2][2])
    # frame 0 id 3: fewer than k kept points in all
    assert 0 < int(stats[0][3][3]) < KNN
    # frame 1 id 1: all twelve position bits, every point kept, lists on both sides of the small cap
    big = vp[1][1]
    assert 3072 < len(big) <= 4096 and int(stats[1][1][3]) == len(big)
    cnt1, sel1 = selection_profile(big, range(0, len(big), 9))
    assert cnt1.max() > min(NBCAPS) and cnt1.max() <= 64 and (sel1 >= KNN).any()
    # frame 2 id 1: the generic surface reaches the list pass too
    cnt2, sel2 = selection_profile(vp[2][1], range(0, len(vp[2][1]), 8))
    assert (sel2 >= KNN).any()
    return cnt, sel
