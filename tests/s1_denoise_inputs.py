"""Small adversarial inputs of the S1 denoise edge tests (test_gpu_s1_denoise_edges.py, test_s1_witness_cpu.py)
and the conditions they must meet, asserted from the witness alone (s1_witness.py; no oracle or device result
enters).  Three frames of 160 x 120:

  frame 0  the slots below on a fronto-parallel wall at z = 0.75 under fx = fy = 64 and the identity pose:
           the points are exact multiples of s = 3 * 2^-8 (wider than a voxel, so every pixel is its own voxel
           mean), and two points are eps-neighbours at eps = 0.04 iff their pixel offset has
           dx^2 + dy^2 <= 11 (eps^2 / s^2 = 11.65; no offset gives 12).  No slot is 32 pixels wide or high: at
           32 lattice steps from the slot's minimum (p - vmin) / voxel is the integer 38.
  frame 1  the same segmentation under a pose that turns the camera by 90 degrees about its axis and
           translates it, with the depth jittered by +-1e-4: the same topology without the lattice's exact
           ties, and the row-major (original) order runs along the other world axis
  frame 2  a tilted, jittered surface under a general rotation (several pixels may share a voxel), with random
           drop-out: borders and noise as they come

The slots of frames 0 and 1 (pixel offsets are (row, column); "block" = a filled rectangle, every point of it
a core point for min_points <= 6; a "spike" = one pixel attached to a block's side, a core point too):

  id 1   contested border, the lower cluster first in space: a block of 18 with a spike (cluster 0, it owns
         pixel (0, 0)), three columns right of the spike one pixel b, three columns further the spike of a
         block of 79 (cluster 1).  b has three eps-neighbours (itself, the two spikes).  n = 100: cluster 0
         has 19 points and 0.2 n = 20, so b's label decides whether 19 more points survive the class filter
         (ndbscan 100, or 81 were b to join cluster 1)
  id 2   the same with the lower cluster later in space: the block of 18 on the right starts a row above the
         block of 79 on the left, so it still owns the first row-major core point
  id 3   three clusters' spikes around one pixel b.  With min_points = 4, b (four eps-neighbours) is a core
         point and joins them into one cluster: a non-core point has at most min_points - 2 other neighbours, so
         no border point is adjacent to three clusters below min_points = 5.  With min_points = 6 (a parameter
         variant of the tests), b is a border point adjacent to three clusters, and n = 38: cluster 0 has 7
         points and 0.2 n = 7.6, so b's label again decides ndbscan (38, or 31)
  id 4   class counts on the limit: three components of 20, 19 and 61 points, n = 100: the class of 20 equals
         0.2 n and is kept, the class of 19 is dropped
  id 5   a border point whose only core neighbour is a spike
  id 6   noise kept, on the limit: a block of 40 and 10 isolated pixels five columns or rows apart, n = 50
  id 7   noise kept, above the limit: a block of 30 and 15 isolated pixels
  id 8   all noise: 30 isolated pixels; all are kept, and every k-NN lies beyond eps
  id 9   25 pixels at z = 2^-4 that share one voxel;  id 10: 40 pixels there that share two voxels

The scene is every slot's voxel means, two jittered copies of them (one jittered by a few centimetres along
every axis, one kept within the thin depth range of frame 1's slots), and a clump of 30 points around one
point of frame 1, so some query has more than ball_k points in its ball.  A wall of frame 0 has one z, so its
crop box is empty by the strict comparison: its slots end with ncovered = 0; frames 1 and 2 reach the query.
"""
import numpy as np

import s1_witness as W

H, Wd = 120, 160
MIN_CLASSES = [0, 2, 4, 5, 6]
NBCAPS = [64, 2]  # 2: below min_points - 1, so border points take the cell walk where they pick their cluster
# the parameter variants, in the witness's argument names
VARIANTS = {"default": {}, "min_points_3": dict(min_points=3), "min_points_6": dict(min_points=6),
            "eps_0.03": dict(eps=0.03), "eps_0.05": dict(eps=0.05), "frac_0.5": dict(frac=0.5),
            "frac_0": dict(frac=0.0), "k_1": dict(k=1), "k_8": dict(k=8), "k_19": dict(k=19),
            "std_ratio_0.5": dict(std_ratio=0.5)}
# (row, column) origin of each slot's drawing
ORIGIN = {1: (0, 0), 2: (0, 20), 3: (0, 40), 4: (0, 62), 5: (0, 90), 6: (20, 0), 7: (20, 25), 8: (20, 50),
          9: (50, 0), 10: (50, 10)}
# id -> the pixel b whose label is contested, relative to the slot's origin
CONTESTED = {1: (2, 6), 2: (3, 9)}
THREE_WAY = {3: (3, 6)}
ONE_SPIKE = {5: (2, 8)}


def _drawing(i):
    """the pixels (row, column) of slot i, relative to its origin"""
    def block(r0, c0, h, w):
        return [(r, c) for r in range(r0, r0 + h) for c in range(c0, c0 + w)]
    if i == 1:
        big = [p for p in block(0, 10, 10, 8) if p != (9, 17)]
        return block(0, 0, 6, 3) + [(2, 3), (2, 6), (2, 9)] + big
    if i == 2:
        return block(0, 13, 6, 3) + [(3, 12), (3, 9), (3, 6)] + block(1, 0, 13, 6) + [(14, 0)]
    if i == 3:  # b at (3, 6); clusters: left 6 + spike, right 16 + spike, bottom 12 + spike
        return (block(2, 0, 2, 3) + [(3, 3), (3, 6), (3, 9)] + block(2, 10, 4, 4) + [(6, 6)] + block(7, 5, 4, 3))
    if i == 4:
        return (block(0, 0, 5, 4) + [p for p in block(0, 8, 5, 4) if p != (4, 11)] + block(0, 16, 10, 6) + [(10, 16)])
    if i == 5:
        return block(0, 0, 5, 5) + [(2, 5), (2, 8)]
    if i == 6:
        return block(0, 0, 5, 8) + [(r, c) for r in (10, 15) for c in range(0, 25, 5)]
    if i == 7:
        return block(0, 0, 5, 6) + [(r, c) for r in (10, 15, 20) for c in range(0, 25, 5)]
    if i == 8:
        return [(r, c) for r in range(0, 25, 5) for c in range(0, 30, 5)]
    if i == 9:
        return block(0, 0, 5, 5)
    if i == 10:
        return block(0, 0, 5, 8)
    raise KeyError(i)


def _pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    R = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
         @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def denoise_inputs():
    """(scene, depth, seg, intrinsics, poses)"""
    rng = np.random.default_rng(23)
    depth = np.zeros((3, H, Wd), np.float32)
    seg = np.zeros((3, H, Wd), np.uint8)
    K = np.tile(np.array([64.0, 64.0, 80.0, 60.0]), (3, 1))
    T = np.tile(np.eye(4), (3, 1, 1))
    T[1] = [[0, -1, 0, 0.3], [1, 0, 0, -0.7], [0, 0, 1, 1.1], [0, 0, 0, 1]]
    T[2] = _pose(0.3, -0.5, 0.8, [0.5, -0.25, 2.0])
    for f in (0, 1):
        depth[f] = 0.75
        for i, (r0, c0) in ORIGIN.items():
            for r, c in _drawing(i):
                assert seg[f, r0 + r, c0 + c] == 0
                seg[f, r0 + r, c0 + c] = i
                if i >= 9:
                    depth[f, r0 + r, c0 + c] = 0.0625
    depth[1] = (depth[1] * (1.0 + rng.uniform(-1e-4, 1e-4, (H, Wd)))).astype(np.float32)
    u = np.arange(Wd)[None, :]
    v = np.arange(H)[:, None]
    depth[2] = (0.8 + 0.002 * u + 0.001 * v + rng.normal(0.0, 0.002, (H, Wd))).astype(np.float32)
    seg[2, 10:34, 10:30] = np.where(rng.random((24, 20)) < 0.5, 1, 0)
    seg[2, 10:40, 40:70] = np.where(rng.random((30, 30)) < 0.25, 2, 0)
    seg[2, 50:70, 10:32] = 3
    seg[2, 50:74, 50:70] = np.where(rng.random((24, 20)) < 0.12, 4, 0)
    seg[2, 50:62, 50:62] = 4
    # the scene
    means = []
    for f in range(3):
        for i in np.unique(seg[f]):
            p = W.world_points(depth[f], seg[f], K[f], T[f], i) if i else ()
            if len(p) >= 25:
                means.append((f, int(i), W.voxel_means(p)[0].astype(np.float64)))
    pts = np.concatenate([m for _, _, m in means])
    thin = np.array([0.003, 0.003, 2e-5])
    centre = next(m for f, i, m in means if (f, i) == (1, 4))[30]
    scene = np.concatenate([pts, pts + rng.normal(0.0, 0.003, pts.shape), pts + rng.normal(0.0, 1.0, pts.shape) * thin,
                            centre + rng.uniform(-1.0, 1.0, (30, 3)) * thin])
    return scene.astype(np.float32), depth, seg, K, T


def witness_reference(inp, **prm):
    """the witness's slots of every frame under the parameters prm"""
    scene, depth, seg, K, T = inp
    return W.frames(scene, depth, seg, K, T, **prm)


def _index_of(slot, seg, i, rc):
    """the voxel number of slot i's pixel at offset rc (every pixel of frames 0 and 1 is its own voxel)"""
    r0, c0 = ORIGIN[i]
    vv, uu = np.nonzero(seg == i)
    hit = np.nonzero((vv == r0 + rc[0]) & (uu == c0 + rc[1]))[0]
    assert len(hit) == 1 and slot["nvox"] == slot["npix"] == len(vv)
    return int(hit[0])


def _adjacent_clusters(slot, eps, min_points):
    """per non-core point with a core neighbour: the sorted cluster numbers of its core neighbours"""
    db = W.dbscan(slot["means"], eps, min_points)
    assert np.array_equal(db["labels"], slot["labels"])
    out = {}
    for b in np.nonzero(~db["core"])[0]:
        nb = db["adj"][b] & db["core"]
        if nb.any():
            out[int(b)] = sorted(set(db["labels"][nb].tolist()))
    return out, db


def _space_key(slot, eps):
    """per point: its cell of edge 1.01 eps from the slot's minimum, packed x-major (the order of a cell grid)"""
    m = slot["means"].astype(np.float64)
    c = np.floor((m - m.min(axis=0)) / (1.01 * eps)).astype(np.int64)
    return (c[:, 0] << 42) | (c[:, 1] << 21) | c[:, 2]


def profile(ref, **prm):
    """what the witness's frames ref hold under the parameters prm: counts of each condition"""
    p = dict(W.DEFAULTS, **prm)
    rep = dict(contested=0, contested_deciding=0, lower_first=0, lower_later=0, three_way=0, one_core=0, on_limit=0,
               one_below=0, noise_kept=0, noise=0, border=0, all_noise=0, one_voxel=0, two_voxels=0, queried=0,
               aabb=0, over_ball_k=0, slots=0)
    for fr in ref:
        for s in fr.values():
            if s["npix"] < p["few_points"]:
                continue
            rep["slots"] += 1
            n = s["nvox"]
            lim = p["frac"] * n  # float64, as the filter computes it
            count = np.bincount(s["labels"] + 1)
            adjc, db = _adjacent_clusters(s, p["eps"], p["min_points"])
            key = _space_key(s, p["eps"])
            rep["noise"] += int(count[0])
            rep["border"] += len(adjc)
            rep["one_core"] += sum(1 for b in adjc if (db["adj"][b] & db["core"]).sum() == 1)
            for b, cl in adjc.items():
                if len(cl) < 2:
                    continue
                rep["contested"] += 1
                rep["three_way"] += len(cl) >= 3
                got = int(s["labels"][b])
                assert got == cl[0]
                # the receiving class is kept with b and dropped without it
                rep["contested_deciding"] += bool(not (count[got + 1] < lim) and (count[got + 1] - 1 < lim))
                first = [key[(s["labels"] == c) & db["core"]].min() for c in cl[:2]]
                rep["lower_first"] += bool(first[0] < first[1])
                rep["lower_later"] += bool(first[0] > first[1])
            rep["on_limit"] += int((count[1:] == lim).sum())
            rep["one_below"] += int((count[1:] == lim - 1).sum())
            if count[0] and not (count[0] < lim):
                rep["noise_kept"] += 1
                rep["all_noise"] += count[0] == n
            rep["one_voxel"] += n == 1 and s["nsor"] == 0
            rep["two_voxels"] += n == 2 and s["nsor"] == 0
            if s["q32"] is not None:
                rep["queried"] += 1
                rep["aabb"] += s["margins"]["aabb"]
                rep["over_ball_k"] += s["most"] > p["ball_k"]
    return rep


def check_inputs(inp, ref=None, **prm):
    """the conditions on the inputs under the parameters prm, from the witness alone; returns (profile,
    smallest margins).  No decision sits on a knife edge under any parameters; the slots' conditions are
    asserted for the parameters under which the drawing meets them (see the module's text)."""
    ref = witness_reference(inp, **prm) if ref is None else ref
    slots = [s for fr in ref for s in fr.values()]
    assert W.knife_edges(slots) == [], W.knife_edges(slots)
    rep = profile(ref, **prm)
    p = dict(W.DEFAULTS, **prm)
    seg = inp[2]
    if p["eps"] == 0.04 and p["min_points"] == 4 and p["frac"] == 0.2:
        for f in (0, 1):
            for i, rc in CONTESTED.items():
                s = ref[f][i]
                b = _index_of(s, seg[f], i, rc)
                adjc, db = _adjacent_clusters(s, p["eps"], p["min_points"])
                assert adjc[b] == [0, 1] and db["adj"][b].sum() == 3 and s["labels"][b] == 0, (f, i)
                n = s["nvox"]
                count = np.bincount(s["labels"] + 1)
                assert n == 100 and count[1] == 20 == np.ceil(0.2 * n) and not (count[1] < 0.2 * n) and count[1] - 1 < 0.2 * n
                assert s["ndbscan"] == 100, (f, i)  # 81 were b to join cluster 1
            s = ref[f][4]
            assert sorted(np.bincount(s["labels"] + 1)[1:].tolist()) == [19, 20, 61] and s["ndbscan"] == 81, f
            assert 0.2 * s["nvox"] == 20.0
            s = ref[f][5]
            b = _index_of(s, seg[f], 5, ONE_SPIKE[5])
            adjc, db = _adjacent_clusters(s, p["eps"], p["min_points"])
            assert adjc[b] == [0] and (db["adj"][b] & db["core"]).sum() == 1 and s["labels"][b] == 0, f
            for i, noise, n in ((6, 10, 50), (7, 15, 45), (8, 30, 30)):
                s = ref[f][i]
                assert s["nvox"] == n and (s["labels"] == -1).sum() == noise and s["ndbscan"] == n, (f, i)
                assert not (noise < 0.2 * n)
            assert 0.2 * 50 == 10.0  # id 6's noise class sits on the limit
            assert (ref[f][9]["nvox"], ref[f][9]["nsor"]) == (1, 0) and (ref[f][10]["nvox"], ref[f][10]["nsor"]) == (2, 0)
        assert rep["contested"] >= 4 and rep["contested_deciding"] >= 4
        assert rep["lower_first"] >= 1 and rep["lower_later"] >= 1
        assert rep["one_core"] >= 2 and rep["on_limit"] >= 2 and rep["one_below"] >= 2
        assert rep["noise_kept"] >= 6 and rep["all_noise"] >= 2 and rep["one_voxel"] >= 2 and rep["two_voxels"] >= 2
        if p["k"] > 1:  # (k = 1: every point's nearest point is itself, its value 0, and nothing survives)
            assert rep["queried"] >= 1 and rep["aabb"] >= 1 and rep["over_ball_k"] >= 1
        else:
            assert rep["queried"] == 0
    if p["eps"] == 0.04 and p["min_points"] == 6 and p["frac"] == 0.2:
        for f in (0, 1):
            s = ref[f][3]
            b = _index_of(s, seg[f], 3, THREE_WAY[3])
            adjc, db = _adjacent_clusters(s, p["eps"], p["min_points"])
            assert adjc[b] == [0, 1, 2] and s["labels"][b] == 0, f
            n = s["nvox"]
            count = np.bincount(s["labels"] + 1)
            assert n == 38 and count[1] == 8 and not (8 < 0.2 * n) and 7 < 0.2 * n and s["ndbscan"] == 38, f  # else 31
        assert rep["three_way"] >= 2
    return rep, W.smallest_margins(slots)
