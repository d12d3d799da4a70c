"""A plain high-precision witness of S1 (turn_mask_to_point: back-project, voxel down-sample, DBSCAN, class
filter, statistical outlier removal, crop, ball query), numpy only.

Written from the reference's Python (utils/mask_backprojection.py:17-151, utils/geometry.py:9-24) and the
published behaviour of the library calls it makes; it shares no code with oracle/s1_oracle.c, with
tests/golden/make_s1_golden.py or with the kernels, and imports none of them.  It is a witness of the
algorithms, not of rounding orders: distances and statistics are taken in np.longdouble in whatever order
numpy sums them.  So that a comparison with a float64 implementation is still exact, every decision also
reports how far it sits from its boundary (the knife-edge report, `margins` of a slot):

  voxel  per voxelised pixel and axis, the distance of (p - vmin) / voxel from an integer
  eps    per point pair, |d2 - eps2| / eps2
  sor    per point of the outlier statistics with a positive value v, |v - thr| / thr
  ball   per query-candidate pair, |d2 - r2| / r2
  aabb   the number of scene coordinates equal to a bound of the crop box (allowed: the crop is strict by
         definition, and strict here)

A decision nearer than MARGIN_F64 (the float64 stages: a handful of float64 roundings is about 1e-15, a
sequential float64 sum over at most 4096 terms about 1e-12) or MARGIN_F32 (the float32 ball distance: the
float32 FMA expression differs from the float64 value by about 5 * 2^-24 relative) is a knife-edge decision;
inputs are chosen so that there are none (knife_edges() == 0).  Two exact ties are structural and not
counted: a slot of one kept point (its value is 0, and 0 < v fails whatever the threshold), and a slot of two
kept points (both values are the same half distance d / 2, the mean (v + v) / 2 = v and the deviation 0 are
exact in any order, so v < thr fails exactly).  Values of 0 (sor_neighbors = 1: the nearest point is the
point itself) are decided by 0 < v alone.
"""
import numpy as np

LD = np.longdouble
MARGIN_F64 = 1e-9
MARGIN_F32 = 1e-5

DEFAULTS = dict(voxel=0.01, eps=0.04, min_points=4, frac=0.2, k=20, std_ratio=2.0, ball_radius=0.01, ball_k=20,
                coverage=0.3, few_points=25, depth_trunc=20.0)
# the witness's argument names -> the fields of mc_bp_params / orc_bp_params
PARAM_FIELDS = dict(voxel="voxel_size", eps="dbscan_eps", min_points="dbscan_min_points",
                    frac="component_min_fraction", k="sor_neighbors", std_ratio="sor_std_ratio",
                    ball_radius="ball_radius", ball_k="ball_k", coverage="coverage_threshold",
                    few_points="few_points", depth_trunc="depth_trunc")
STAT_NAMES = ["id", "npix", "nvox", "ndbscan", "nsor", "ncovered", "nneighbors", "kept"]
_CHUNK = 256


def abi_params(prm):
    """the witness's parameters under their mc_bp_params field names"""
    return {PARAM_FIELDS[k]: v for k, v in prm.items()}


def world_points(depth, seg, K, T, mask_id, depth_trunc=20.0):
    """the world points of the pixels with seg == mask_id and 0 < depth < depth_trunc, row-major, float64
    (a pinhole camera fx, fy, cx, cy at depth scale 1, then the 4 x 4 camera-to-world pose)"""
    depth = np.asarray(depth, np.float32)
    fx, fy, cx, cy = np.asarray(K, np.float64).reshape(4)
    T = np.asarray(T, np.float64).reshape(4, 4)
    z64 = depth.astype(np.float64)
    v, u = np.nonzero((np.asarray(seg) == mask_id) & (z64 > 0) & (z64 < depth_trunc))
    z = z64[v, u]
    cam = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z, np.ones_like(z)], axis=1)
    w = cam @ T.T
    return w[:, :3] / w[:, 3:4]


def voxel_means(p, voxel=0.01):
    """voxel_down_sample: (per-voxel means [nv, 3] longdouble in order of each voxel's first point, the voxel
    number of every point, the smallest distance of any (p - vmin) / voxel from an integer)"""
    t = (p - (p.min(axis=0) - voxel / 2)) / voxel
    ix = np.floor(t).astype(np.int64)
    margin = float(np.abs(t - np.rint(t)).min())
    _, first, inv = np.unique(ix, axis=0, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    order = np.argsort(first, kind="stable")          # voxels by their first point
    number = np.empty(len(first), np.int64)
    number[order] = np.arange(len(first))
    vox = number[inv]
    means = np.zeros((len(first), 3), LD)
    pl = p.astype(LD)
    for j in range(len(first)):
        means[j] = pl[vox == j].sum(axis=0) / LD((vox == j).sum())
    return means, vox, margin


def _d2_rows(p, a, b, q=None):
    """squared distances [b - a, n] of points a .. b of p (or of q) to every point of p, in p's precision"""
    q = p if q is None else q
    d2 = 0
    for c in range(3):
        s = q[a:b, c, None] - p[None, :, c]
        d2 = d2 + s * s
    return d2


def dbscan(p, eps=0.04, min_points=4):
    """DBSCAN as published (Ester et al. 1996, the variant Open3D and scikit-learn implement, points seeded
    in index order): p [n, 3] longdouble -> dict(labels, core, adj (the n x n predicate d2 < eps2, self
    included), margin)"""
    n = len(p)
    e2 = LD(eps) * LD(eps)
    adj = np.zeros((n, n), bool)
    margin = np.inf
    for a in range(0, n, _CHUNK):
        d2 = _d2_rows(p, a, min(a + _CHUNK, n))
        adj[a:a + _CHUNK] = d2 < e2
        margin = min(margin, float((np.abs(d2 - e2) / e2).min()))
    core = adj.sum(axis=1) >= min_points
    labels = np.full(n, -1, np.int64)
    c = 0
    for i in range(n):                                 # clusters: the connected components of the core points,
        if not core[i] or labels[i] >= 0:              # numbered by their smallest member
            continue
        labels[i] = c
        todo = [i]
        while todo:
            q = todo.pop()
            new = np.nonzero(adj[q] & core & (labels < 0))[0]
            labels[new] = c
            todo.extend(new.tolist())
        c += 1
    for i in np.nonzero(~core)[0]:                     # border points: the smallest adjacent cluster number
        nb = adj[i] & core
        if nb.any():
            labels[i] = labels[nb].min()
    return dict(labels=labels, core=core, adj=adj, margin=margin)


def class_filter(labels, frac=0.2):
    """indices of the points whose label class (noise is a class) is not smaller than frac * n"""
    n = len(labels)
    count = np.bincount(labels + 1)
    return np.nonzero(~(count[labels + 1] < frac * n))[0]


def knn_means(p, k):
    """per point of p [m, 3]: the mean of its min(k, m) smallest distances, itself included"""
    m = len(p)
    kk = min(k, m)
    v = np.zeros(m, p.dtype)
    for a in range(0, m, _CHUNK):
        d2 = _d2_rows(p, a, min(a + _CHUNK, m))
        v[a:a + _CHUNK] = np.sqrt(np.partition(d2, kk - 1, axis=1)[:, :kk]).sum(axis=1) / kk
    return v


def sor_keep(v, std_ratio=2.0):
    """remove_statistical_outlier's decision from the points' k-NN mean distances v: (keep flags, threshold)"""
    m = len(v)
    pos = v > 0
    mean = v[pos].sum() / m
    if m < 2:
        return np.zeros(m, bool), v.dtype.type(np.nan)
    std = np.sqrt(np.where(pos, (v - mean) ** 2, 0).sum() / (m - 1))
    thr = mean + std_ratio * std
    return pos & (v < thr), thr


def sor(p, k=20, std_ratio=2.0):
    """statistical outlier removal on the points p [m, 3] longdouble -> dict(keep, v, thr, margin)"""
    m = len(p)
    if m == 0 or k < 1:
        return dict(keep=np.zeros(m, bool), v=np.zeros(m, LD), thr=LD(np.nan), margin=np.inf)
    v = knn_means(p, k)
    keep, thr = sor_keep(v, std_ratio)
    margin = np.inf
    if m > 2 and (v > 0).any():
        margin = float((np.abs(v[v > 0] - thr) / thr).min())
    return dict(keep=keep, v=v, thr=thr, margin=margin)


def crop(q32, scene32):
    """ids of the scene points strictly inside the float32 AABB of q32, and how many scene coordinates
    equal one of its bounds"""
    lo, hi = q32.min(axis=0), q32.max(axis=0)
    inside = ((scene32 > lo) & (scene32 < hi)).all(axis=1)
    return np.nonzero(inside)[0], int(((scene32 == lo) | (scene32 == hi)).sum())


def ball_hits(q32, scene32, cand, radius=0.01):
    """the predicate d2 < float32(radius)^2 [nq, ncand] with d2 in float64, and its margin"""
    r2 = np.float64(np.float32(radius)) ** 2
    q = q32.astype(np.float64)
    c = scene32[cand].astype(np.float64)
    hit = np.zeros((len(q), len(c)), bool)
    margin = np.inf
    if len(c):
        for a in range(0, len(q), _CHUNK):
            d2 = _d2_rows(c, a, min(a + _CHUNK, len(q)), q)
            hit[a:a + _CHUNK] = d2 < r2
            margin = min(margin, float((np.abs(d2 - r2) / r2).min()))
    return hit, margin


def ball_query(q32, scene32, radius=0.01, ball_k=20):
    """crop and ball query -> dict(cand, aabb, covered, points (sorted unique scene ids), most (the largest
    number of candidates in one ball, before the cut to ball_k), margin)"""
    cand, aabb = crop(q32, scene32)
    hit, margin = ball_hits(q32, scene32, cand, radius)
    taken = hit & (np.cumsum(hit, axis=1) <= ball_k)   # the first ball_k in index order
    return dict(cand=cand, aabb=aabb, covered=int(hit.any(axis=1).sum()), points=cand[taken.any(axis=0)].astype(np.int32),
                most=int(hit.sum(axis=1).max()) if hit.size else 0, margin=margin)


def slot(scene32, depth, seg, K, T, mask_id, voxel=0.01, eps=0.04, min_points=4, frac=0.2, k=20, std_ratio=2.0,
         ball_radius=0.01, ball_k=20, coverage=0.3, few_points=25, depth_trunc=20.0):
    """one mask id of one frame through every stage; the stages it did not reach stay at 0 / None"""
    r = dict(id=int(mask_id), npix=0, nvox=0, ndbscan=0, nsor=0, ncovered=0, nneighbors=0, kept=0, points=None,
             world=None, means=None, labels=None, core=None, filtered=None, sor=None, q32=None, most=0,
             margins=dict(voxel=np.inf, eps=np.inf, sor=np.inf, ball=np.inf, aabb=0))
    p = world_points(depth, seg, K, T, mask_id, depth_trunc)
    r["world"], r["npix"] = p, len(p)
    if len(p) < few_points:
        return r
    means, _, r["margins"]["voxel"] = voxel_means(p, voxel)
    r["means"], r["nvox"] = means, len(means)
    db = dbscan(means, eps, min_points)
    r["labels"], r["core"], r["margins"]["eps"] = db["labels"], db["core"], db["margin"]
    idx = class_filter(db["labels"], frac)
    r["filtered"], r["ndbscan"] = idx, len(idx)
    so = sor(means[idx], k, std_ratio)
    r["sor"], r["margins"]["sor"] = so, so["margin"]
    r["nsor"] = int(so["keep"].sum())
    if r["nsor"] < few_points:
        return r
    q32 = means[idx[so["keep"]]].astype(np.float64).astype(np.float32)
    r["q32"] = q32
    bq = ball_query(q32, scene32, ball_radius, ball_k)
    r["ncovered"], r["most"] = bq["covered"], bq["most"]
    r["margins"]["ball"], r["margins"]["aabb"] = bq["margin"], bq["aabb"]
    if bq["covered"] / len(q32) < coverage:
        return r
    r["points"], r["nneighbors"], r["kept"] = bq["points"], len(bq["points"]), 1
    return r


def frames(scene, depth, seg, K, T, **prm):
    """every frame's slots, {mask id: slot}, ids ascending; scene is cast to float32 as the graph stage does"""
    scene32 = np.asarray(scene, np.float64).astype(np.float32).reshape(-1, 3)
    out = []
    for f in range(len(depth)):
        ids = [int(i) for i in np.unique(seg[f]) if i != 0]
        out.append({i: slot(scene32, depth[f], seg[f], K[f], T[f], i, **prm) for i in ids})
    return out


def stats_row(s):
    return [s[c] for c in STAT_NAMES]


def knife_edges(slots):
    """the decisions of these slots that sit inside their margin: a list of (id, stage, margin)"""
    bad = []
    for s in slots:
        for stage, lim in (("voxel", MARGIN_F64), ("eps", MARGIN_F64), ("sor", MARGIN_F64), ("ball", MARGIN_F32)):
            if s["margins"][stage] < lim:
                bad.append((s["id"], stage, s["margins"][stage]))
    return bad


def smallest_margins(slots):
    """{stage: the smallest margin over these slots}"""
    return {st: min([s["margins"][st] for s in slots] + [np.inf]) for st in ("voxel", "eps", "sor", "ball")}
