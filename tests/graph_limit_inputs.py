"""Inputs of the graph-path limit tests (test_gpu_graph_limits.py), the branch each is meant to take, and
a plain numpy restatement of S2/S3 -- all checked without a GPU by test_graph_limit_inputs_cpu.py.

The graph path accepts 16384 frames and 2047 masks in a frame.  Which kernel, table and window a mask
gets is decided by constants in maskclustering_amd/csrc (mc_graph_plan.hpp, mc_s3_kernels.inl,
mc_s4_kernels.inl); they are restated here (test_graph_limit_inputs_cpu.py reads the sources and fails if
one was retuned), and every builder's scene comes with the predicate of its branch computed from the
scene itself: `route()` gives, for a mask, the kernel (wave / workgroup), the number of non-boundary points T,
of touched frames, of distinct (frame, mask) pairs its points meet, the path (hash / dense) and the windows.

`s3_restatement` is written from the text of the reference's graph/construction.py (build_point_in_mask_matrix
:34-62, process_one_mask :98-135, the undo :164-169) on the dense uint16 matrix; it imports nothing from
oracle/.  It is pinned to the reference's own outputs on the golden cases."""
import numpy as np

from maskclustering_amd.synthetic import SceneMasks, make_scene

MAX_FRAMES, MAX_PER_FRAME, MAX_MASKS = 16384, 2047, 262144   # mc_scene_set_masks
LOCAL_BITS = 12                                              # list entry = frame << 12 | mask-in-frame
S3_WAVE = dict(W=1, FWMAX=32, CNT=1024, HS=512)              # S3Cfg<1>
S3_BIG = dict(W=4, FWMAX=256, CNT=4096, HS=2048)             # S3Cfg<kS3BigW>, kS3BigW = 4
S3_SMALL_PTS = 1024                                          # kS3SmallPts
HIST_REPLICA_BYTES = 40 * 1024                               # kHistReplicaBytes
HIST_TILES_LDS = 2 * 64 * 8 * 8                              # the two staged 64 x 8-word tiles of k_s4_hist
THR_STATIC_LDS = 256 * 8 + 20 * 4                            # kS4ThrStaticLds
TEST_WORDS = 4                                               # kTestWords (k6_pairs)


# ---------------------------------------------------------------------------------------------------
# host decisions, restated (mc_graph_plan.hpp)
# ---------------------------------------------------------------------------------------------------
def s3_wave_ok(F, max_per_frame):
    return F <= 64 * S3_WAVE["FWMAX"] and max_per_frame < S3_WAVE["CNT"]


def hist_stride(F):
    return (F + 1) | 1


def hist_replicas(F):
    R = 32
    while R > 1 and R * hist_stride(F) * 4 > HIST_REPLICA_BYTES:
        R >>= 1
    return R


def hist_replica_fits(F):
    return hist_replicas(F) * hist_stride(F) * 4 <= HIST_REPLICA_BYTES


def hist_lds_bytes(F):
    return HIST_TILES_LDS + hist_replicas(F) * hist_stride(F) * 4


def thresholds_lds_bytes(F):
    return 8 * (F + 1) + THR_STATIC_LDS


def max_per_frame(scene):
    return int(np.bincount(scene.mask_col, minlength=max(scene.num_frames, 1)).max()) if scene.num_masks else 0


# ---------------------------------------------------------------------------------------------------
# scenes as frame lists
# ---------------------------------------------------------------------------------------------------
def frame_lists(scene, offset=0):
    """frames[c] = [(label, points + offset), ...] of a scene (the inverse of from_frame_lists)"""
    frames = [[] for _ in range(scene.num_frames)]
    for g in range(scene.num_masks):
        frames[int(scene.mask_col[g])].append((int(scene.mask_label[g]), scene.mask_points(g) + offset))
    return frames


def add_mask(frames, c, pts):
    """a further mask in frame c under the next free label; returns (c, label)"""
    label = max((lb for lb, _ in frames[c]), default=0) + 1
    frames[c].append((label, np.asarray(pts, np.int32)))
    return c, label


def global_index(scene, c, label):
    g = np.nonzero((scene.mask_col == c) & (scene.mask_label == label))[0]
    assert len(g) == 1
    return int(g[0])


def well_formed(scene):
    """what mc_scene_set_masks asks of its input, and what the builders here promise on top (no empty mask,
    so no skipped frame: input order == global order)"""
    col, lab, off, pts = scene.mask_col, scene.mask_label, scene.mask_off, scene.mask_pts
    assert scene.num_frames <= MAX_FRAMES and scene.num_masks <= MAX_MASKS and max_per_frame(scene) <= MAX_PER_FRAME
    assert np.all(np.diff(col) >= 0) and (not len(col) or (col[0] >= 0 and col[-1] < scene.num_frames))
    assert np.all(lab >= 1) and np.all(lab <= 65535) and np.all(np.diff(off) >= 1) and off[0] == 0
    assert len(np.unique(col.astype(np.int64) * 65536 + lab)) == len(col), "duplicate label in a frame"
    assert pts.min() >= 0 and pts.max() < scene.num_points and off[-1] == len(pts)
    g_of = np.repeat(np.arange(len(col), dtype=np.int64), np.diff(off))
    assert len(np.unique(g_of * scene.num_points + pts)) == len(pts), "a mask's points must be unique"
    return True


# ---------------------------------------------------------------------------------------------------
# S2 restated sparsely (the per-point lists the S3 kernels walk) and the S3 routing of a mask
# ---------------------------------------------------------------------------------------------------
def point_lists(scene):
    """(boundary [P] bool, pt_off [P + 1], entries sorted by point): entry = frame << 12 | mask-in-frame"""
    P, F, col = scene.num_points, scene.num_frames, scene.mask_col
    g_of = np.repeat(np.arange(scene.num_masks), np.diff(scene.mask_off))
    fs = np.searchsorted(col, np.arange(F + 1))
    frame = col[g_of].astype(np.int64)
    slot = g_of - fs[frame]
    pts = scene.mask_pts.astype(np.int64)
    order = np.argsort(pts * F + frame, kind="stable")
    ks = (pts * F + frame)[order]
    same = ks[1:] == ks[:-1]
    dup = np.zeros(len(ks), bool)
    dup[1:] |= same
    dup[:-1] |= same
    bnd = np.zeros(P, bool)
    bnd[pts[order][dup]] = True
    pt_off = np.zeros(P + 1, np.int64)
    np.cumsum(np.bincount(pts, minlength=P), out=pt_off[1:])
    return bnd, pt_off, ((frame << LOCAL_BITS) | slot)[order]


def route(scene, g, lists, wave_ok=None):
    """the branch of mask g in k_s3_masks, from the inputs alone"""
    bnd, pt_off, ent = lists
    fs = np.searchsorted(scene.mask_col, np.arange(scene.num_frames + 1))
    if wave_ok is None:
        wave_ok = s3_wave_ok(scene.num_frames, max_per_frame(scene))
    p = scene.mask_points(g)
    V = p[~bnd[p]]
    e = np.unique(np.concatenate([ent[pt_off[q]:pt_off[q + 1]] for q in V])) if len(V) else np.zeros(0, np.int64)
    frames = np.unique(e >> LOCAL_BITS)
    wave = bool(wave_ok and len(p) <= S3_SMALL_PTS)
    cfg = S3_WAVE if wave else S3_BIG
    dense = len(e) > cfg["HS"]          # a table that fills up: more distinct pairs than HS
    if dense:                           # windows: the longest prefix of touched frames whose counters fit in CNT
        windows, n, used = [], 0, 0
        for nm in (fs[frames + 1] - fs[frames]):
            if n and (used + nm > cfg["CNT"] or n == 64 * cfg["W"]):
                windows.append(n)
                n, used = 0, 0
            n, used = n + 1, used + int(nm)
        if n:
            windows.append(n)
    else:
        windows = [min(64 * cfg["W"], len(frames) - j) for j in range(0, len(frames), 64 * cfg["W"])]
    return dict(g=g, size=len(p), T=len(V), kernel="wave" if wave else "workgroup", touched=len(frames),
                pairs=len(e), path="dense" if dense else "hash", windows=windows,
                max_slot=int((e & ((1 << LOCAL_BITS) - 1)).max()) if len(e) else -1,
                max_frame=int(frames.max()) if len(frames) else -1)


# ---------------------------------------------------------------------------------------------------
# S2 + S3 restated on the dense matrix, from the reference's text
# ---------------------------------------------------------------------------------------------------
def dense_matrices(scene):
    """build_point_in_mask_matrix (:34-62): (kept masks, boundary [P], point_in_mask [P, F] u16,
    point_frame [P, F] bool).  A frame without points is skipped (:50-51): its masks are not in the global
    list.  A point in two masks of a frame is a boundary point and reads 0 in that frame (:56, :61)."""
    P, F = scene.num_points, scene.num_frames
    lens = np.diff(scene.mask_off)
    frame_pts = np.bincount(scene.mask_col, weights=lens, minlength=max(F, 1))
    kept = np.nonzero(frame_pts[scene.mask_col] > 0)[0]
    g_of = np.repeat(np.arange(scene.num_masks), lens)
    frame = scene.mask_col[g_of].astype(np.int64)
    pts = scene.mask_pts.astype(np.int64)
    pim = np.zeros((P, F), np.uint16)
    pfm = np.zeros((P, F), bool)
    pim[pts, frame] = scene.mask_label[g_of]
    pfm[pts, frame] = True
    key, cnt = np.unique(pts * max(F, 1) + frame, return_counts=True)
    twice = key[cnt > 1]
    pim[twice // max(F, 1), twice % max(F, 1)] = 0
    bnd = np.zeros(P, bool)
    bnd[twice // max(F, 1)] = True
    return kept, bnd, pim, pfm


def decide(T, nz, bc, mvt, cont):
    """one frame of process_one_mask (:116-130) from its three counts: 0 not visible, 1 split, 2 contained"""
    c0 = np.int64(T - nz)
    tot = np.int64(T)
    if 1 - c0 / tot < mvt and tot - c0 < 500:
        return 0
    return 2 if np.int64(bc) / np.int64(nz) > cont else 1


def s3_restatement(scene, mvt, ust, cont, rows=None, dense=None, detail=None):
    """process_masks (:98-170) for the kept masks `rows` (None: all of them; otherwise the masks they are
    contained in are evaluated too, for the undo needs to know whether those are under-segmented).
    Returns rows, boundary (point ids), vf [len(rows), F] bool, the contained entries (c_row, c_col: global
    mask ids, sorted), the under-segmented ids among rows; `detail`, a dict, receives
    (g, frame) -> (T, nz, bc, label of the argmax) of every possibly visible frame."""
    kept, bnd, pim, pfm = dense if dense is not None else dense_matrices(scene)
    F, M = scene.num_frames, len(kept)
    col, lab = scene.mask_col[kept], scene.mask_label[kept]
    index = {(int(c), int(lb)): i for i, (c, lb) in enumerate(zip(col, lab))}   # global_frame_mask_list.index

    def process_one_mask(i):
        p = scene.mask_points(kept[i])
        info = pim[p[~bnd[p]], :]                                   # :105-108
        frames, tgts = [], []
        visible = split = 0
        for f in np.where(np.sum(info, axis=0, dtype=np.int64) > 0)[0]:   # :110
            count = np.bincount(info[:, f])                         # :116
            invisible_ratio = count[0] / np.sum(count)
            nz = np.sum(count) - count[0]
            if detail is not None:
                c2 = count.copy()
                c2[0] = 0
                detail[(i, int(f))] = (len(info), int(nz), int(c2.max()), int(np.argmax(c2)))
            if 1 - invisible_ratio < mvt and nz < 500:              # :119
                continue
            visible += 1
            count[0] = 0
            best = int(np.argmax(count))                            # the smallest id on ties
            if count[best] / np.sum(count) > cont:                  # :124-128
                frames.append(int(f))
                tgts.append(index[(int(f), best)])
            else:
                split += 1
        return not (visible == 0 or split / visible > ust), frames, tgts   # :132

    ids = list(range(M)) if rows is None else [int(i) for i in rows]
    res = {i: process_one_mask(i) for i in ids}
    valid = {i: r[0] for i, r in res.items()}
    for t in sorted({t for r in res.values() for t in r[2]} - set(res)):
        valid[t] = process_one_mask(t)[0]
    vf = np.zeros((len(ids), F), bool)
    c_row, c_col = [], []
    for k, i in enumerate(ids):
        for f, t in zip(res[i][1], res[i][2]):
            if valid[t]:                                            # the undo (:164-169) drops the others
                vf[k, f] = True
                c_row.append(i)
                c_col.append(t)
    order = np.lexsort((c_col, c_row))
    return dict(rows=np.asarray(ids, np.int32), kept=kept, boundary=np.nonzero(bnd)[0].astype(np.int32), vf=vf,
                c_row=np.asarray(c_row, np.int32)[order], c_col=np.asarray(c_col, np.int32)[order],
                undersegment=np.asarray([i for i in ids if not valid[i]], np.int32), pim=pim, pfm=pfm)


def dense_keys(pim, pfm):
    """the dense entries of GraphRun.canonical() from the two matrices"""
    nzp, nzc = np.nonzero(pim)
    return dict(pim_p=nzp.astype(np.int32), pim_c=nzc.astype(np.int32), pim_v=pim[nzp, nzc].astype(np.int32),
                pfm_bits=np.packbits(pfm, axis=1))


# ---------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------
CFG = dict(mask_visible_threshold=0.3, undersegment_filter_threshold=0.3, view_consensus_threshold=0.9,
           contained_threshold=0.8)


def _objects(scene):
    """the generator's objects: contiguous point ranges, recovered from the masks' point ids"""
    K = scene.meta["num_objects"]
    rng = np.random.default_rng(scene.meta["seed"])
    cuts = np.sort(rng.choice(np.arange(1, scene.num_points), size=K - 1, replace=False))
    return np.concatenate([[0], cuts]), np.concatenate([cuts, [scene.num_points]])


def case_a(extra_frame):
    """F = 2048, the last size of the wave kernel; with one frame added (a copy of frame 1000's masks) the
    first size at which every mask goes to the workgroup kernel"""
    frames = frame_lists(make_scene(6000, 2048, 40, 0.02, seed=1))
    if extra_frame:
        frames.append([(lb, m.copy()) for lb, m in frames[1000]])
    return SceneMasks.from_frame_lists(6000, frames), CFG


def _wide_scene(F, picks, seed=1):
    """a make_scene scene of 40 objects and narrow frame windows in the first F - len(picks) frames, and one
    wide mask in each of the last frames: picks = [(objects, points per object or None for all)]"""
    base = make_scene(6000, F - len(picks), 40, 0.02, seed=seed)
    starts, ends = _objects(base)
    frames = frame_lists(base)
    for objs, per in picks:
        pts = np.concatenate([np.arange(starts[o], ends[o] if per is None else min(ends[o], starts[o] + per))
                              for o in objs])
        frames.append([(1, pts)])
    s = SceneMasks.from_frame_lists(6000, frames)
    return s, [global_index(s, F - len(picks) + k, 1) for k in range(len(picks))]


def case_b():
    """F = 2112: masks of more than 1024 points that touch more than 256 and more than 512 frames and meet
    fewer than 2048 pairs: the hash path of the workgroup kernel over two and more windows"""
    s, wide = _wide_scene(2112, [(range(2, 9), None), (range(1, 40, 3), None), ((23, 25, 26, 28, 33, 35, 38), None)])
    return s, dict(CFG, mask_visible_threshold=0.05), wide


def case_c():
    """as case_b with masks that meet more than 2048 pairs: s3_dense<4> over several windows"""
    s, wide = _wide_scene(2112, [(range(40), 30), (range(40), None), (range(5, 40), 40)])
    return s, dict(CFG, mask_visible_threshold=0.02, contained_threshold=0.4), wide


CROWD_FRAMES = (3, 4, 10, 11, 12, 20)


def case_d(n, seed=3):
    """24 frames; frames 3, 4, 10, 11, 12 and 20 cut the points [0, 2n) into n masks of two points each (pairs
    (2j, 2j + 1) in frames 3, 10 and 20; shifted by one point in the others), under labels permuted against the
    slot order; the points from 4096 carry a small make_scene scene.  n = 1023: the last count at which the
    wave kernel runs, 1024: the first all-workgroup count, 2047: the most a frame may hold.
    d': frame 0 holds a mask of the points [0, 4000) (workgroup kernel), frame 1 one of [100, 1100) (the wave
    kernel where it runs) and frame 2 one of [2000, 2600): they meet every mask of the crowded frames, so they
    overflow their tables and take s3_dense with windows of one to four frames."""
    assert 2 * n + 1 <= 4096
    rng = np.random.default_rng(seed)
    frames = frame_lists(make_scene(1904, 24, 24, 0.12, seed=seed), offset=4096)
    for k, c in enumerate(CROWD_FRAMES):
        labels = rng.permutation(n) + 1
        sh = k % 2
        frames[c] = [(int(labels[j]), np.array([2 * j + sh, 2 * j + 1 + sh])) for j in range(n)]
    wide = [add_mask(frames, 0, np.arange(0, 4000)), add_mask(frames, 1, np.arange(100, 1100)),
            add_mask(frames, 2, np.arange(2000, 2600))]
    s = SceneMasks.from_frame_lists(6000, frames)
    return s, dict(CFG, contained_threshold=0.0), [global_index(s, c, lb) for c, lb in wide]


SEEN = 1024  # points of a mask seen in every frame (case e)


def case_e(F, seed=2):
    """masks seen in every frame at F = 5200 (one histogram replica) and F = 16384 (not even one fits
    kHistReplicaBytes).  Points [3900, 4924) are set A, [4924, 5948) set D.  Frames 0, 1 and 2 each hold a
    mask of all of A and one of all of D; every later frame f holds a two-point mask {A[i], D[i]},
    i = f * 1024 // F (the last frame leaves D[i] out).  With mask_visible_threshold = 0.0009 one point of
    1024 makes a mask visible, so the three A masks are seen and contained in all F frames and the three
    D masks in F - 1: observer counts F (9 ordered pairs) and F - 1 (27).  The two-point masks are seen only
    in the few frames that share their points (and split between A and D in frames 0 to 2, which the
    under-segmentation threshold 0.9 lets pass), so the contained entries stay near 20 F; at F = 16384 each
    point serves 16 frames, so the two-point masks of a point merge in the first iteration (the oracle's S6
    took 5 s of CPU when they did not).  The points below 3900 carry a make_scene scene of narrow windows."""
    assert F >= 2 * SEEN
    frames = frame_lists(make_scene(3900, F, 20, 8.0 / F, seed=seed))
    A, D = np.arange(3900, 3900 + SEEN), np.arange(3900 + SEEN, 3900 + 2 * SEEN)
    wide = []
    for c in range(3):
        wide.append(add_mask(frames, c, A))
        wide.append(add_mask(frames, c, D))
    for f in range(3, F):
        i = f * SEEN // F
        add_mask(frames, f, [A[i]] if f == F - 1 else [A[i], D[i]])
    s = SceneMasks.from_frame_lists(6000, frames)
    return s, dict(CFG, mask_visible_threshold=0.0009, undersegment_filter_threshold=0.9), \
        [global_index(s, c, lb) for c, lb in wide]


def case_f(F, seed):
    """random level-0 nodes for mc_nodes_set + mc_cluster_run: visible frames in a window of 300 frames per
    node (windows reach the last frame), a few contained masks each"""
    rng = np.random.default_rng(seed)
    N, M = 300, 240
    vf = np.zeros((N, F), bool)
    start = rng.integers(0, F - 300 + 1, N)
    start[:4] = F - 300
    for i in range(N):
        vf[i, start[i]:start[i] + 300] = rng.random(300) < 0.2
    vf[0, F - 1] = vf[1, F - 1] = True
    vf[2], vf[3] = True, True          # two nodes seen in every frame
    cm = rng.random((N, M)) < 0.03
    return vf, cm, [6.0, 3.0, 1.5, 1.0], [0.9, 0.5, 1.0][seed % 3]


def case_g():
    """rows for mc_observer_thresholds at F = 16384: name -> [rows, F] bool"""
    F = MAX_FRAMES
    ones, one_bit, last = np.ones((1, F), bool), np.zeros((1, F), bool), np.zeros((1, F), bool)
    one_bit[0, 777] = True
    last[0, F - 1] = True
    rng = np.random.default_rng(4)
    mixed = np.concatenate([np.repeat(ones, 9, 0), np.repeat(last, 7, 0), np.repeat(one_bit, 5, 0),
                            rng.random((40, F)) < 0.3])
    mixed[9 + 7 + 5:, F - 1] = True
    return dict(all_ones=np.repeat(ones, 3, 0), one_bit=np.repeat(one_bit, 3, 0), last_bit=np.repeat(last, 3, 0),
                mixed=mixed)


# ---------------------------------------------------------------------------------------------------
# S3 decisions that sit exactly on a rule
# ---------------------------------------------------------------------------------------------------
KNIFE_CFGS = {  # mask_visible_threshold, undersegment_filter_threshold, contained_threshold
    "A": (0.3, 0.5, 0.8),
    "B": (0.2, 0.5, 0.4),
    "C": (0.5, 0.5, 0.8),
}


def knife_scene(pad_frames=0):
    """Masks Q (frame 0, disjoint point blocks) and, in the later frames, masks that cover chosen numbers of
    Q's points.  Returns (scene, edges): edges[name] = (label of Q in frame 0, frame, config, T, nz, bc, want)
    with want the decision 0 / 1 / 2 the rule gives there.  pad_frames appends frames without masks (F above
    the wave kernel's limit sends every mask to the workgroup kernel).

      vis_up    T = 10, nz = 3, mvt = 0.3: 1 - 7/10 is one ulp above 0.3: visible
      vis_down  T = 5, nz = 1, mvt = 0.2: 1 - 4/5 is one ulp below 0.2: not visible
      nz499/500 T = 1700 (workgroup size) and T = 1010 (wave size, mvt = 0.5): below the visible ratio, 499
                points are not visible and 500 are
      cont_eq   nz = 5, bc = 4, contained_threshold = 0.8: 4/5 == 0.8 is not above it: split
      tie       two masks with 3 points each, slot order (label 7, label 2): np.argmax takes label 2
      useg_eq   a mask visible in 4 frames and split in 2 of them: 2/4 == 0.5 is not above it: kept; its
                neighbour split in 2 of 3 is under-segmented"""
    frames = [[] for _ in range(8)]
    edges, nxt = {}, [0]

    def block(n):
        nxt[0] += n
        return np.arange(nxt[0] - n, nxt[0])

    def q_mask(n):
        pts = block(n)
        return pts, add_mask(frames, 0, pts)[1]

    q, lb = q_mask(10)
    add_mask(frames, 1, q[:3])
    edges["vis_up"] = (lb, 1, "A", 10, 3, 3, 2)
    q, lb = q_mask(5)
    add_mask(frames, 1, q[:1])
    edges["vis_down"] = (lb, 1, "B", 5, 1, 1, 0)
    q, lb = q_mask(1700)
    add_mask(frames, 1, q[:499])
    add_mask(frames, 2, q[:500])
    edges["nz499_workgroup"] = (lb, 1, "A", 1700, 499, 499, 0)
    edges["nz500_workgroup"] = (lb, 2, "A", 1700, 500, 500, 2)
    q, lb = q_mask(1010)
    add_mask(frames, 1, q[:499])
    add_mask(frames, 2, q[:500])
    edges["nz499_wave"] = (lb, 1, "C", 1010, 499, 499, 0)
    edges["nz500_wave"] = (lb, 2, "C", 1010, 500, 500, 2)
    q, lb = q_mask(5)
    add_mask(frames, 1, q[:4])
    add_mask(frames, 1, q[4:5])
    add_mask(frames, 2, np.concatenate([q[:5], block(1)]))
    edges["cont_eq"] = (lb, 1, "A", 5, 5, 4, 1)
    edges["cont_above"] = (lb, 2, "A", 5, 5, 5, 2)
    q, lb = q_mask(6)
    frames[3] += [(7, q[:3]), (2, q[3:])]
    edges["tie"] = (lb, 3, "B", 6, 6, 3, 2)
    # under-segmentation: visible in frame 0 (itself) and frames 4..6 (4..5 for the second), split in two of them
    for name, nvis in (("useg_eq", 4), ("useg_above", 3)):
        q, lb = q_mask(8)
        for c in range(4, 3 + nvis):
            if c < 6:
                add_mask(frames, c, q[:4])
                add_mask(frames, c, q[4:])
            else:
                add_mask(frames, c, q)
        edges[name] = (lb, None, "A", nvis, 2, None, name == "useg_above")
    frames[7].append((1, block(3)))   # the last frame holds a mask
    frames += [[] for _ in range(pad_frames)]
    return SceneMasks.from_frame_lists(nxt[0], frames), edges


# ---------------------------------------------------------------------------------------------------
# the scenes by name, built once and left unchanged, and the branch each must take
# ---------------------------------------------------------------------------------------------------
SCENES = {
    "a2048": lambda: case_a(False) + ([],), "a2049": lambda: case_a(True) + ([],),
    "b": case_b, "c": case_c,
    "d1023": lambda: case_d(1023), "d1024": lambda: case_d(1024), "d2047": lambda: case_d(2047),
    "e5200": lambda: case_e(5200), "e16384": lambda: case_e(16384),
}
_built = {}


def built(name):
    """(scene, config, wide masks) of a case; the arrays are read-only"""
    if name not in _built:
        s, cfg, wide = SCENES[name]()
        for a in (s.mask_col, s.mask_label, s.mask_off, s.mask_pts):
            a.setflags(write=False)
        _built[name] = (s, cfg, tuple(wide))
    return _built[name]


def check_branch(name):
    """asserts, from the inputs alone, that the case sits on the branch it is meant to pin; returns the
    figures (F, M, most masks in a frame, the wide masks' routes)"""
    s, cfg, wide = built(name)
    assert well_formed(s) and s.num_points <= 6000
    F, M, mpf = s.num_frames, s.num_masks, max_per_frame(s)
    FW = (F + 63) // 64
    lists = point_lists(s)
    R = [route(s, g, lists) for g in wide]
    sizes = np.diff(s.mask_off)
    last_frame_used = int(s.mask_col[-1]) == F - 1
    if name == "a2048":       # the last size of the wave kernel: bit 63 of word 31 is a frame with masks
        assert F == 64 * S3_WAVE["FWMAX"] and s3_wave_ok(F, mpf) and not s3_wave_ok(F + 1, mpf) and last_frame_used
        assert (sizes <= S3_SMALL_PTS).any()
    elif name == "a2049":     # one more frame: word 32 exists and holds one frame, no mask takes the wave kernel
        assert F == 64 * S3_WAVE["FWMAX"] + 1 and FW == 33 and not s3_wave_ok(F, mpf) and s3_wave_ok(F - 1, mpf)
        assert last_frame_used
    elif name == "b":
        assert all(r["kernel"] == "workgroup" and r["size"] > S3_SMALL_PTS and r["path"] == "hash"
                   and r["pairs"] < S3_BIG["HS"] for r in R)
        assert any(256 < r["touched"] <= 512 for r in R) and any(r["touched"] > 512 for r in R)
        assert sorted(len(r["windows"]) for r in R)[0] == 2 and max(len(r["windows"]) for r in R) >= 4
        assert max(r["max_frame"] for r in R) == F - 1 and FW == 33
    elif name == "c":
        assert all(r["kernel"] == "workgroup" and r["size"] > S3_SMALL_PTS and r["path"] == "dense"
                   and r["pairs"] > S3_BIG["HS"] and r["touched"] > 512 and len(r["windows"]) >= 3 for r in R)
    elif name.startswith("d"):
        n = int(name[1:])
        assert mpf == n and all(r["path"] == "dense" for r in R[:2]) and R[2]["path"] == "hash"
        assert R[0]["kernel"] == "workgroup" and R[0]["pairs"] > S3_BIG["HS"]
        assert max(r["max_slot"] for r in R) >= min(n - 1, 1999)      # slots near the frame's last are carried
        if n == 1023:         # the wave kernel still runs; its counters hold one crowded frame per window
            assert s3_wave_ok(F, mpf) and not s3_wave_ok(F, mpf + 1)
            assert R[1]["kernel"] == "wave" and R[1]["pairs"] > S3_WAVE["HS"] and R[1]["windows"].count(1) >= 5
            assert R[2]["kernel"] == "wave"
        else:
            assert not s3_wave_ok(F, mpf) and all(r["kernel"] == "workgroup" for r in R)
        if n == 1024:         # the first count that ends the wave kernel; several crowded frames per window
            assert s3_wave_ok(F, mpf - 1) and max(R[0]["windows"]) >= 4
        if n == 2047:         # the most a frame may hold: two crowded frames fill CNT, a third does not fit
            assert n == MAX_PER_FRAME and 2 * n <= S3_BIG["CNT"] < 3 * n
            assert {1, 2} <= set(R[0]["windows"]) and max(R[0]["windows"][1:]) == 2
    elif name.startswith("e"):
        assert all(r["path"] == "dense" and r["touched"] in (F, F - 1) and r["max_frame"] >= F - 2 for r in R)
        assert sorted(r["touched"] for r in R) == [F - 1] * 3 + [F] * 3
        if name == "e5200":   # one replica, which fits; two would not
            assert hist_replicas(F) == 1 and hist_replica_fits(F) and 2 * hist_stride(F) * 4 > HIST_REPLICA_BYTES
        else:                 # the most frames: not even one replica fits, the frame bitmaps are full
            assert F == MAX_FRAMES and FW == S3_BIG["FWMAX"] and not hist_replica_fits(F)
            assert hist_lds_bytes(F) > 64 * 1024 and thresholds_lds_bytes(F) > 64 * 1024
            assert all(len(r["windows"]) == 64 for r in R)
    return dict(F=F, M=M, max_per_frame=mpf, routes=R)
