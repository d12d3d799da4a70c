"""Inputs of the S1 ring-search tests (test_gpu_s1_ring.py) and the conditions they must meet, asserted from the
inputs and the witness alone (s1_witness.py; no oracle or device result enters; test_s1_ring_inputs_cpu.py asserts
the same without a GPU).  k_bp_knn_ring (mc_bp_denoise.inl, mc_bp_ring.hpp) serves the deferred points of a slot:
the kept points with fewer than k = 20 eps-neighbours, or with more than MC_BP_NBCAP.  A deferred point settles
at R = 1 (its k-th kept neighbour of the 27 cells around its own lies within one cell edge ce = 1.01 eps), at
R = 2 (the 125 cells, within 2 ce) or by a scan of the slot's whole cloud.  ring_profile restates that in numpy
on the slot's grid: cells of edge ce from the origin min(world points) - voxel / 2.  Two frames of 160 x 120:

  frame 0  a fronto-parallel wall at z = 0.75 under fx = fy = 64 and the identity pose: points on an exact
           lattice of step 3 * 2^-8 (every pixel its own voxel), eps-neighbours iff dx^2 + dy^2 <= 11 pixels, a
           cell edge 3.45 pixels; squared distances tie exactly
    id 1   30 x 31 pixels with 35 % left out at random: edges and holes defer points, which settle at R = 2,
           some with one of their k nearest in a shell cell and an exact tie at the k-th distance across cells
           (no slot of the wall is 32 pixels wide or high: at 32 lattice steps from the slot's minimum
           (p - vmin) / voxel is the integer 38, a knife edge of the voxel stage)
    id 2   a block of 6 x 6: 36 kept points and 72 buckets under the 125 cells of a search (collisions within
           a ring are certain); its corners are deferred, in the slot's cell 0 and in its last cell
    id 3 .. 7  blocks of 25, 40, 54, 30 and 56 points, consecutive slots: a wave of the ring kernel holds points
           of several slots and grids
    id 8   30 isolated pixels, all noise and all kept: every point goes to the whole cloud
    id 9   three small clusters around one pixel (s1_denoise_inputs.py's id 3): 38 kept, R = 2 and whole cloud
    id 10  a block of 12 x 12: its interior points have 37 eps-neighbours, over MC_BP_NBCAP = 30, and settle at
           R = 1
  frame 1  a tilted, jittered surface (no ties) under a translated pose
    id 1   58 x 58 pixels: more than 3072 voxels, so the slot runs in the 4096 class and its deferred points (the
           rim) queue to the ring kernel from there
    id 2   30 x 30 pixels with 75 % left out: sparse, deferred throughout
"""
import numpy as np

import s1_witness as W

H, Wd = 120, 160
EPS, KNN, VOXEL = 0.04, 20, 0.01
MIN_CLASSES = [0, 2, 5, 6]
NBCAPS = [64, 30]
BLOCKS = {3: (5, 5), 4: (5, 8), 5: (6, 9), 6: (5, 6), 7: (7, 8)}


def ring_inputs():
    """(scene, depth, seg, intrinsics, poses)"""
    rng = np.random.default_rng(29)
    depth = np.zeros((2, H, Wd), np.float32)
    seg = np.zeros((2, H, Wd), np.uint8)
    K = np.tile(np.array([64.0, 64.0, 80.0, 60.0]), (2, 1))
    T = np.tile(np.eye(4), (2, 1, 1))
    T[1, :3, 3] = [0.5, -0.25, 2.0]
    depth[0] = 0.75
    seg[0, 0:30, 0:31] = np.where(rng.random((30, 31)) < 0.65, 1, 0)
    seg[0, 50:56, 0:6] = 2
    c0 = 10
    for i, (h, w) in BLOCKS.items():
        seg[0, 50:50 + h, c0:c0 + w] = i
        c0 += w + 4
    seg[0, 70:95:5, 0:30:5] = 8
    for r, c in ([(r, c) for r in (2, 3) for c in (0, 1, 2)] + [(3, 3), (3, 6), (3, 9)] +
                 [(r, c) for r in range(2, 6) for c in range(10, 14)] + [(6, 6)] +
                 [(r, c) for r in range(7, 11) for c in range(5, 8)]):
        seg[0, 70 + r, 60 + c] = 9
    seg[0, 100:112, 0:12] = 10
    u = np.arange(Wd)[None, :]
    v = np.arange(H)[:, None]
    depth[1] = (0.8 + 0.002 * u + 0.001 * v + rng.normal(0.0, 0.002, (H, Wd))).astype(np.float32)
    seg[1, 2:60, 2:60] = 1
    seg[1, 70:100, 70:100] = np.where(rng.random((30, 30)) < 0.25, 2, 0)
    pts = [W.world_points(depth[f], seg[f], K[f], T[f], i) for f in range(2) for i in np.unique(seg[f]) if i]
    return np.concatenate(pts).astype(np.float32), depth, seg, K, T


def witness_reference(inp):
    scene, depth, seg, K, T = inp
    return W.frames(scene, depth, seg, K, T)


def oracle_reference(inp):
    """the oracle's (labels, off, pts, stats) of every frame, read-only"""
    from oracle import oracle
    scene, depth, seg, K, T = inp
    ref = oracle.s1_frames(np.asarray(scene, np.float64).astype(np.float32), list(depth), list(seg), K, T)
    for out in ref:
        for a in out:
            a.setflags(write=False)
    return ref


def ring_profile(slot, nbcap, eps=EPS, k=KNN, voxel=VOXEL):
    """per deferred point of a witness slot (kept, and fewer than k or more than nbcap eps-neighbours among the
    kept points): dict(idx, settle (1, 2 or 0 = the whole cloud), cell, cmax, shell (one of its k nearest lies in
    a shell cell), tie (its k-th and (k + 1)-th distances are equal bit for bit, in different cells))"""
    p = slot["means"][slot["filtered"]].astype(np.float64)
    ce = 1.01 * eps
    origin = slot["world"].min(axis=0) - voxel / 2
    cell = np.floor((p - origin) / ce).astype(np.int64)
    out = dict(idx=[], settle=[], cell=[], shell=[], tie=[], cmax=cell.max(axis=0), kept=len(p))
    for i in range(len(p)):
        d = p[i] - p
        d2 = ((d[:, 0] * d[:, 0]) + (d[:, 1] * d[:, 1])) + (d[:, 2] * d[:, 2])
        cnt = int((d2 < eps * eps).sum())
        if not (cnt < k or cnt > nbcap):
            continue
        cheb = np.abs(cell - cell[i]).max(axis=1)
        settle, shell, tie = 0, False, False
        for R in (1, 2):
            o = np.argsort(d2[cheb <= R], kind="stable")
            dd, cc = d2[cheb <= R][o], cheb[cheb <= R][o]
            reach = R * ce
            if len(dd) >= k and dd[k - 1] < reach * reach * (1.0 - 1e-9):
                settle = R
                shell = bool((cc[:k] == 2).any())
                if len(dd) > k and dd[k] == dd[k - 1]:
                    cl = cell[cheb <= R][o]
                    tie = bool((cl[k] != cl[k - 1]).any())
                break
        out["idx"].append(i)
        out["settle"].append(settle)
        out["cell"].append(cell[i])
        out["shell"].append(shell)
        out["tie"].append(tie)
    for key in ("idx", "settle", "shell", "tie"):
        out[key] = np.asarray(out[key])
    out["cell"] = np.asarray(out["cell"]).reshape(-1, 3)
    return out


def check_inputs(inp, ref=None):
    """the conditions on the inputs, from the inputs and the witness alone; returns the counts"""
    ref = witness_reference(inp) if ref is None else ref
    slots = [s for fr in ref for s in fr.values()]
    assert W.knife_edges(slots) == [], W.knife_edges(slots)
    prof = {(f, i, cap): ring_profile(s, cap) for f, fr in enumerate(ref) for i, s in fr.items() for cap in NBCAPS}
    rep = dict(r1=0, r2=0, cloud=0, shell=0, tie=0)
    for (f, i, cap), pr in prof.items():
        if cap == min(NBCAPS):
            rep["r1"] += int((pr["settle"] == 1).sum())
        else:
            rep["r2"] += int((pr["settle"] == 2).sum())
            rep["cloud"] += int((pr["settle"] == 0).sum())
            rep["shell"] += int(pr["shell"].sum())
            rep["tie"] += int(pr["tie"].sum())
    # settling: at least 10 deferred points each way
    assert rep["r1"] >= 10 and rep["r2"] >= 10 and rep["cloud"] >= 10, rep
    assert (prof[(0, 10, 30)]["settle"] == 1).sum() >= 10 and len(prof[(0, 10, 64)]["idx"]) < 144
    assert (prof[(0, 8, 64)]["settle"] == 0).sum() == 30
    p9 = prof[(0, 9, 64)]
    assert p9["kept"] == 38 and (p9["settle"] == 2).sum() == 21 and (p9["settle"] == 0).sum() == 17
    # collisions: the 125 cells of a search outnumber the slot's 2 n buckets
    p2 = prof[(0, 2, 64)]
    assert p2["kept"] == 36 and 2 * ref[0][2]["nvox"] < 125 and len(p2["idx"]) >= 4 and (p2["settle"] == 2).all()
    # grid edges: deferred points in cell 0 or 1 on every axis (their neighbour cells lie at -1 and -2), and in
    # the slot's last cell
    for key in ((0, 2, 64), (0, 1, 64)):
        pr = prof[key]
        assert (pr["cell"] <= 1).all(axis=1).any() and (pr["cell"] == pr["cmax"]).all(axis=1).any(), key
    # (the tilted slot: three axes of several cells, deferred points in the first and the last cell of each)
    big = prof[(1, 1, 64)]
    assert (big["cmax"] >= 2).all() and (big["cell"] == 0).any(axis=0).all() and (big["cell"] == big["cmax"]).any(axis=0).all()
    assert all((prof[(0, 1, 64)]["cell"][:, a] == 0).any() for a in range(3))
    # a shell cell holds one of the k nearest; an exact tie at the k-th distance across two cells
    assert rep["shell"] >= 10 and rep["tie"] >= 1, rep
    assert prof[(0, 1, 64)]["tie"].any()
    # mixed waves: consecutive slots of 20 to 60 points, each with deferred points
    for i, (h, w) in BLOCKS.items():
        assert ref[0][i]["nvox"] == h * w and 20 <= h * w <= 60 and len(prof[(0, i, 64)]["idx"]) >= 4, i
    # the 3072-and-up class queues to the ring kernel
    assert 3072 < ref[1][1]["nvox"] <= 4096 and len(prof[(1, 1, 64)]["idx"]) >= 10
    assert len(prof[(1, 2, 64)]["idx"]) >= 10
    return rep
