"""Inputs that take post-processing (mc_pp_run, mc_pp_run_device: csrc/mc_pp_*.inl) past
one frame word, past its object windows, to its node-size threshold, past its slot count and onto its rules.
Pure numpy.  test_pp_limit_inputs_cpu.py asserts without a GPU that every case reaches what it is for;
test_gpu_pp_limits.py compares the device with oracle/pp_oracle.py on them, bit for bit.

The sizes the cases sit on are read out of the sources (constants()), never retyped, so a retuned constant moves
the cases with it or fails the CPU test.

Coordinates are multiples of U = 2^-10 m unless a case says otherwise: every difference, square and sum of a
distance is then exact in float64, d^2 is an integer number of U^2 and eps^2 = 10485.76 U^2 is none, so no pair
sits on eps and no summation order can matter.

  case            input                                                            reaches
  f65 .. f200     nodes with 1, 63, 64, 65 (129) visible frames of F, masks in     FW 2, 2, 3, 4; W 1, 2, 3; frame
                  the first, last, 64th, 65th, 128th, 129th visible frame and in   ranks 63, 64, 127, 128; points
                  columns 63, 64, 127, 128; points seen in no visible frame        kept and dropped; cvid = 0
  shifted         f65 moved by (2^17, -2^16, 2^15) m                               the same result as f65
  obj257          nodes of kPPBoxChunk + 1 clusters of 4 points, one with a        kPPBoxChunk + 1 and + 2 objects;
                  stray point; masks over the objects round the window edge        boxes / kept counts at the edge
  obj1025,        the same with kPPObjChunk + 1 and 2 kPPObjChunk + 1 clusters;    2 and 3 windows of mask counters;
  obj2049         masks that tie across windows, inside a window, and win late     the first maximum of each tie
  n8192, n8193    a node of kPPLdsUF (+ 1) points: a connected lattice, two small  no / one node of the split DBSCAN
                  clusters, a stray point; nodes of 511, 512, 513 points           (17 items); 1, 1, 2 items at 500
  slots17, 40     17 / 40 nodes over one blob, near-duplicates of each other       a point in 17 / 40 kept objects
  wide            two clusters 2^21 - 2 and 2^21 - 1 DBSCAN cells apart            accepted / MC_ERR_UNSUPPORTED
  edges/...       one tiny scene per side of each rule (EDGE_PAIRS)                results differ pair by pair
"""
import functools
import os
import re
from typing import NamedTuple

import numpy as np

from oracle import pp_oracle

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskclustering_amd", "csrc")
U = 2.0 ** -10
EPS, MIN_POINTS, RATIO = 0.1, 4, 0.8


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) == 1, f"{what}: {len(m)} matches of {pattern!r}"
    return int(m[0])


@functools.lru_cache(maxsize=None)
def constants():
    """the six constants and k_pp_dbscan's workgroup size, read out of the sources"""
    kern, plan, host = _src("mc_pp_kernels.inl"), _src("mc_pp_plan.hpp"), _src("mc_pp_host.inl")
    c = {n: _one(r"constexpr int %s = (\d+);" % n, kern, n) for n in ("kPPObjChunk", "kPPBoxChunk", "kPPSlots", "kPPLdsUF")}
    c.update({n: _one(r"constexpr int %s = (\d+);" % n, plan, n) for n in ("kPPItemPoints", "kPPMaxKept")})
    c["dbscan_threads"] = _one(r"hipLaunchKernelGGL\(mc::k_pp_dbscan<(\d+)>", host, "k_pp_dbscan launch")
    assert "int big_min = mc::kPPLdsUF;" in host and "> big_min" in plan       # the default threshold, strict
    assert "int sl = mc::kPPSlots;" in host
    return c


def big_items(sizes, big_min):
    """pp_big_items (mc_pp_plan.hpp) restated: (nodes above big_min points, their items of kPPItemPoints points)"""
    ip = constants()["kPPItemPoints"]
    big = [n for n in sizes if n > big_min]
    return len(big), sum(-(-n // ip) for n in big)


class Case(NamedTuple):
    scene: np.ndarray
    pfm: np.ndarray
    mask_pts: list
    mask_col: np.ndarray
    onodes: list
    thr: float
    meta: dict

    @property
    def inputs(self):
        return self.scene, self.pfm, self.mask_pts, self.mask_col, self.onodes


def pack_arrays(scene, pfm, mask_pts, mask_col, onodes):
    """the oracle's inputs as the arrays of mc_pp_run"""
    from maskclustering_amd.utils.post_process import _bits as bits
    F = pfm.shape[1]
    nodes = [n for n in onodes if len(n[0]) >= 2]                    # post_process.py:182
    off = lambda lens: np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)  # noqa: E731
    cat = lambda arrs, dt: np.concatenate(arrs).astype(dt) if arrs else np.zeros(0, dt)  # noqa: E731
    qm = cat([np.asarray(n[0], np.int64) for n in nodes], np.int32)
    return dict(scene=np.ascontiguousarray(scene, np.float64), pfm=bits(pfm, F), F=F,
                moff=off([len(p) for p in mask_pts]), mpts=cat(list(mask_pts), np.int32),
                vf=bits(np.stack([n[1] for n in nodes]), F) if nodes else np.zeros((0, (F + 63) // 64), np.uint64),
                poff=off([len(n[2]) for n in nodes]), pts=cat([n[2] for n in nodes], np.int32),
                qoff=off([len(n[0]) for n in nodes]), qm=qm, qc=np.asarray(mask_col, np.int32)[qm])


class _Scene:
    def __init__(self, F):
        self.F, self.xyz, self.masks, self.cols, self.nodes, self.n = F, [], [], [], [], 0

    def points(self, xyz):
        xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
        ids = np.arange(self.n, self.n + len(xyz), dtype=np.int64)
        self.xyz.append(xyz)
        self.n += len(xyz)
        return ids

    def mask(self, pts, col):
        pts = np.asarray(pts, np.int64).ravel()
        assert len(np.unique(pts)) == len(pts) and 0 <= col < self.F
        self.masks.append(pts)
        self.cols.append(col)
        return len(self.masks) - 1

    def node(self, masks, vf, order):
        vf = np.ones(self.F, bool) if vf is None else np.asarray(vf, bool)
        assert all(vf[self.cols[m]] for m in masks)
        self.nodes.append((list(masks), vf, np.asarray(order, np.int64)))
        return len(self.nodes) - 1

    def hits(self, k):
        """per point of the scene: the frames in which a mask of node k holds it"""
        h = np.zeros((self.n, self.F), bool)
        for m in self.nodes[k][0]:
            h[self.masks[m], self.cols[m]] = True
        return h

    def case(self, pfm, thr, **meta):
        scene = np.concatenate(self.xyz)
        assert pfm.shape == (self.n, self.F) and pfm.dtype == bool
        return Case(scene, pfm, self.masks, np.asarray(self.cols, np.int32), self.nodes, float(thr), meta)


def _square(x, y, z=0.0, s=31):
    """4 points s U apart: each has the other three within eps, so all four are core points"""
    return np.array([[0, 0, 0], [s, 0, 0], [0, s, 0], [s, s, 0]]) * U + np.array([x, y, z], np.float64)


def _lattice(n, nx, ny, origin):
    """the first n points of an nx x ny x (as many as needed) lattice of pitch 51 U (0.0498 m: neighbours along an
    axis at 51 and 102 U, the diagonal at 72 U, all below eps = 102.4 U), layer by layer: connected for every n"""
    i = np.arange(n)
    return np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], axis=1) * (51 * U) + np.asarray(origin, np.float64)


# ---- frame words ------------------------------------------------------------------------------------
def _f_case(F, shift=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(1000 + F)
    s = _Scene(F)
    nvs = [1, 63, 64, 65] + ([129] if F >= 129 else [])
    must = sorted({c for c in (0, 63, 64, 127, 128, F - 1) if c < F})
    node_pts, node_blobs, vcols_of = [], [], []
    for k, nv in enumerate(nvs):
        if nv == 1:
            vcols = np.array([64])
        else:
            rest = np.setdiff1d(np.arange(F), must)
            vcols = np.sort(np.concatenate([must, rng.choice(rest, nv - len(must), replace=False)])).astype(np.int64)
        blobs = []
        for b in range(2 + k % 3):
            off = rng.integers(-45, 46, (400, 3))
            off = off[np.unique(off, axis=0, return_index=True)[1]][:90]
            blobs.append(s.points(off * U + np.array([4.0 * k, 1.0 * b, 0.0])))
        stray = s.points(np.array([[4.0 * k + 0.5, 0.5, 0.5], [4.0 * k + 0.5, 0.5, 1.5]]))   # the noise class
        node_pts.append(np.concatenate(blobs + [stray]))
        node_blobs.append(blobs)
        vcols_of.append(vcols)
    for k, vcols in enumerate(vcols_of):
        blobs, nb = node_blobs[k], len(node_blobs[k])
        cols = [vcols[0], vcols[-1]] + [vcols[r] for r in (63, 64, 127, 128) if r < len(vcols)] + \
               [c for c in (63, 64, 127, 128) if c in vcols]
        cols = sorted(set(int(c) for c in cols))
        while len(cols) < 2 * nb + 1:                              # at least two masks for every blob
            cols.append(int(rng.choice(vcols)))
        masks = []
        for j, c in enumerate(cols):
            b = blobs[j % nb]
            pts = [b[rng.random(len(b)) < rng.uniform(0.5, 0.9)]]
            if j % 3 == 0:
                o = blobs[(j + 1) % nb]
                pts.append(o[rng.random(len(o)) < 0.1])
            other = node_pts[(k + 1) % len(nvs)]
            pts.append(rng.choice(other, 5, replace=False))        # points outside the node
            masks.append(s.mask(np.concatenate(pts), c))
        vf = np.zeros(F, bool)
        vf[vcols] = True
        s.node(masks, vf, rng.permutation(node_pts[k]))
    pfm = rng.random((s.n, F)) < 0.12
    for w in range((F + 63) // 64):                                  # bits in every word of every row
        lo, hi = 64 * w, min(F, 64 * w + 64)
        pfm[np.arange(s.n), rng.integers(lo, hi, s.n)] = True
    for k, vcols in enumerate(vcols_of):                             # points seen in no visible frame of their node
        blind = node_pts[k][rng.random(len(node_pts[k])) < 0.1]
        pfm[np.ix_(blind, vcols)] = False
    c = s.case(pfm, 0.3, vcols=vcols_of)
    return c._replace(scene=c.scene + np.asarray(shift, np.float64))


# ---- object windows ---------------------------------------------------------------------------------
def _obj_case(C):
    """two nodes of C clusters of 4 points (pitch 0.5 m): object o of the first is cluster o; the second has a stray
    point, the noise class, as object 0, so its cluster c is object c + 1"""
    k = constants()
    box, chunk = k["kPPBoxChunk"], k["kPPObjChunk"]
    F = 32
    rng = np.random.default_rng(C)
    s = _Scene(F)
    outside = s.points(np.array([[-9.0, -9.0, 0.0], [-9.0, -8.0, 0.0], [-9.0, -7.0, 0.0]]))
    want_best, nodes_pid = {}, []
    for twin in (0, 1):
        c = np.arange(C)
        corner = np.stack([(c % 64) * 0.5, twin * 64.0 + (c // 64) * 0.5, np.zeros(C)], axis=1)
        pid = s.points((corner[:, None, :] + _square(0, 0)[None, :, :]).reshape(-1, 3)).reshape(C, 4)
        # list order: point 0 of every cluster in cluster order (it numbers the clusters), the others shuffled
        order = np.concatenate([pid[:, 0], rng.permutation(pid[:, 1:].ravel())])
        nobj = C + twin
        if twin:
            stray = s.points(np.array([[-3.0, 64.0, 0.0]]))
            order = np.concatenate([order[:C // 2], stray, order[C // 2:]])

        def pts_of(o, n):
            return stray[:n] if twin and o == 0 else pid[o - twin, :n]

        specs = []                                                    # (object, points) lists, expected object
        for e in (box, chunk, 2 * chunk):                             # the objects round a window edge, in rotation
            g = [o for o in (e - 2, e - 1, e, e + 1) if o < nobj]
            if e >= nobj:
                continue
            for r in range(len(g)):
                specs.append(([(g[(r + i) % len(g)], 4 - i) for i in range(len(g))], g[r]))
        ties = [([(chunk, 3), (5, 3)], 5),                            # (a) a tie across windows: the first
                ([(chunk + 5, 3), (6, 3)], 6),
                ([(7 + 128, 2), (7, 2)], 7),                          # (b) a tie in one lane of one window
                ([(10, 2), (9, 2)], 9),                               #     and in neighbouring lanes
                ([(chunk + 7 + 64, 2), (chunk + 7, 2)], chunk + 7),
                ([(3, 2), (chunk, 3)], chunk),                        # (c) strictly more in a later window
                ([(8, 2), (chunk + 3, 3)], chunk + 3),
                ([(chunk - 1, 1), (chunk, 2)], chunk),                #     the last and first object of two windows
                ([(2 * chunk, 2), (chunk + 11, 2), (11, 2)], 11),
                ([(4, 1), (chunk + 4, 2), (2 * chunk, 3)], 2 * chunk)]
        if nobj > chunk:                                              # those whose objects the node has
            specs += [t for t in ties if all(o < nobj for o, _ in t[0])]
        if twin:
            specs.append(([(1, 1), (0, 1)], 0))                       # the noise point ties with object 1: object 0
        masks = []
        for spec, want in specs:
            pts = np.concatenate([pts_of(o, n) for o, n in spec] + [outside[:1]])
            for _ in range(2):                                        # twice: the chosen object has 2 masks
                m = s.mask(pts, len(s.masks) % F)
                want_best[m] = (twin, want)
                masks.append(m)
        m = s.mask(outside, len(s.masks) % F)                         # holds no point of the node: dropped
        want_best[m] = (twin, -1)
        masks.append(m)
        s.node(masks, None, order)
        nodes_pid.append((pid, stray if twin else None))
    # the ratio: of the points a mask holds, the first 1 + o % 3 of object o are kept (seen exactly where they are
    # hit), the others dropped (seen in more than twice as many frames); thr = 0.5
    pfm = np.zeros((s.n, F), bool)
    for twin, (pid, stray) in enumerate(nodes_pid):
        h = s.hits(twin)
        for cidx in range(C):
            for j in range(4):
                p, cnt = pid[cidx, j], int(h[pid[cidx, j]].sum())
                if cnt == 0:
                    continue
                pfm[p] = h[p]
                if j >= 1 + (cidx + twin) % 3:
                    assert 2 * cnt + 1 <= F
                    pfm[p, np.nonzero(~h[p])[0][:cnt + 1]] = True
        if stray is not None:
            pfm[stray[0]] = h[stray[0]]
    return s.case(pfm, 0.5, want_best=want_best, clusters=C)


# ---- node sizes -------------------------------------------------------------------------------------
def _n_case(N):
    """a node of N points (a connected lattice of N - 9, two 4-point clusters, a stray point) and nodes of one less
    than, exactly and one more than k_pp_dbscan's workgroup size (= kPPItemPoints) points"""
    F = 8
    rng = np.random.default_rng(N)
    s = _Scene(F)
    lat = s.points(_lattice(N - 9, 64, 64, (0.0, 0.0, 0.0)))
    c1, c2 = s.points(_square(-2.0, 0.0)), s.points(_square(-2.0, 2.0))
    stray = s.points(np.array([[-4.0, -4.0, 0.0]]))
    out = s.points(np.array([[-8.0, -8.0, 0.0]]))
    sub = lambda a, f: a[rng.random(len(a)) < f]  # noqa: E731
    masks = [s.mask(sub(lat, 0.6), 0), s.mask(np.concatenate([sub(lat, 0.5), c1]), 1), s.mask(np.concatenate([c1, c2]), 2),
             s.mask(np.concatenate([c2, stray]), 3), s.mask(np.concatenate([stray, sub(lat, 0.1)]), 5), s.mask(c1, 4),
             s.mask(c2, 6), s.mask(stray, 7), s.mask(np.concatenate([stray, out]), 0)]
    s.node(masks, None, rng.permutation(np.concatenate([lat, c1, c2, stray])))
    nt = constants()["dbscan_threads"]
    for j, n in enumerate((nt - 1, nt, nt + 1)):
        p = s.points(_lattice(n, 8, 8, (10.0 * (j + 1), 20.0, 0.0)))
        s.node([s.mask(sub(p, 0.6), 1), s.mask(sub(p, 0.6), 2), s.mask(sub(p, 0.3), 2)], None, rng.permutation(p))
    return s.case(rng.random((s.n, F)) < 0.4, 0.3, sizes=[len(n[2]) for n in s.nodes])


# ---- slots ------------------------------------------------------------------------------------------
def _slots_case(m):
    """m nodes over one blob: its first 20 points in every node, each of the other 40 in every second one, and 3 points
    of the node's own, so the nodes' objects are near-duplicates round the 0.8 overlap; 3 unrelated nodes"""
    F = 8
    rng = np.random.default_rng(m)
    s = _Scene(F)

    def cloud(n, origin):
        off = rng.integers(0, 61, (4 * n, 3))
        return off[np.unique(off, axis=0, return_index=True)[1]][:n] * U + np.asarray(origin, np.float64)

    blob = s.points(cloud(60, (0.0, 0.0, 0.0)))
    for j in range(m):
        own = s.points(cloud(3, (0.0, 0.0, 0.0)))
        pts = np.concatenate([blob[:20], blob[20:][rng.random(40) < 0.50], own])
        masks = [s.mask(pts[rng.random(len(pts)) < 0.92], (j + i) % F) for i in range(2)]
        s.node(masks, None, rng.permutation(pts))
    for j in range(3):
        pts = s.points(cloud(30, (5.0 * (j + 1), 0.0, 0.0)))
        s.node([s.mask(pts[rng.random(30) < 0.8], i) for i in range(3)], None, rng.permutation(pts))
    return s.case(rng.random((s.n, F)) < 0.5, 0.1, blob=blob, nodes=m)


# ---- the extent limit -------------------------------------------------------------------------------
def _wide_case(cells):
    """two 4-point clusters in one node whose extent along x is `cells` DBSCAN cells of 1.01 eps"""
    ce = EPS * 1.01                                                   # pp_check_args: dbscan_eps * 1.01
    ext = np.ceil(cells * ce / U) * U
    assert np.floor(ext / ce) == cells and np.floor((ext - U) / ce) == cells - 1
    s = _Scene(2)
    a, b = s.points(_square(0.0, 0.0)), s.points(_square(ext - 31 * U, 0.0))
    s.node([s.mask(a, 0), s.mask(a[:3], 1), s.mask(b, 0), s.mask(b[1:], 1)], None, np.concatenate([a, b]))
    c = s.case(np.ones((s.n, 2), bool), 0.0, cells=cells)
    assert np.ptp(c.scene[:, 0]) == ext
    return c


# ---- rules ------------------------------------------------------------------------------------------
def _all_seen(s, thr=0.0, **meta):
    return s.case(np.ones((s.n, s.F), bool), thr, **meta)             # ratio = hits / (F + 1e-6): kept when hit


def _edge_eps(near):
    """A has itself, C1, C2 and - only when B is nearer than eps - B within eps: min_points = 4 makes A a core point
    and {A, C1, C2, B} a cluster, or leaves all four noise beside the stray S.  B at 0.1 gives d^2 = 0.1 * 0.1, the
    very double eps^2 is: not a neighbour.  (Not dyadic.)"""
    s = _Scene(2)
    bx = np.nextafter(0.1, 0) if near else 0.1
    g = s.points(np.array([[0, 0, 0], [0, 31 * U, 0], [0, 0, 31 * U], [bx, 0, 0], [3, 3, 3]]))
    d = s.points(_square(5.0, 0.0))
    allp = np.concatenate([g, d])
    s.node([s.mask(allp, 0), s.mask(allp, 1), s.mask(d, 0), s.mask(d, 1)], None, allp)
    return _all_seen(s, bx=bx)


def _edge_border(x_first):
    """Q is within eps of one core point of X (round x = 0) and of Y (round x = 200 U) and has 3 neighbours, so it is
    a border point; it is listed before every core point, and Y's core points before X's unless x_first: Q joins
    the cluster of the smaller number, the one listed first"""
    s = _Scene(2)
    q = s.points(np.array([[100 * U, 0, 0]]))
    yz = np.array([[0, 0, 0], [0, 31, 0], [0, 0, 31], [0, 31, 31]]) * U
    x, y = s.points(yz), s.points(yz + np.array([200 * U, 0, 0]))
    order = np.concatenate([q, x, y] if x_first else [q, y, x])
    yq = np.concatenate([y, q])
    s.node([s.mask(x, 0), s.mask(x, 1), s.mask(yq, 0), s.mask(yq, 1)], None, order)
    return _all_seen(s, q=int(q[0]), x=x, y=y)


def _edge_noise(with_noise):
    """a cluster and, as the last entry of the list, the node's only noise point: object 0 all the same"""
    s = _Scene(2)
    c, n = s.points(_square(0.0, 0.0)), s.points(np.array([[2.0, 0, 0]]))
    allp = np.concatenate([c, n])
    s.node([s.mask(allp, 0), s.mask(allp, 1), s.mask(n, 0), s.mask(n, 1)], None, allp if with_noise else c)
    return _all_seen(s)


def _edge_no_core():
    """a node of three points within eps of each other: nobody has min_points neighbours, so there is no core point
    and no cluster, and the noise class is the node's only object; beside it a node of one cluster and no noise"""
    s = _Scene(2)
    a = s.points(np.array([[0, 0, 0], [0, 31 * U, 0], [0, 0, 31 * U]]))
    b = s.points(_square(5.0, 0.0))
    s.node([s.mask(a, 0), s.mask(a, 1)], None, a)
    s.node([s.mask(b, 0), s.mask(b, 1)], None, b)
    return _all_seen(s)


RATIO_EQ = 1 / (2 + 1e-6)                                             # a point hit in 1 of the 2 frames it is seen in


def _edge_ratio(thr):
    """one cluster of T (1 hit, seen in 2 visible frames), U (1 hit, seen in no visible frame), Z (no hit, seen in
    none) and three points with 2 hits of 2; frame 3 is not visible"""
    s = _Scene(4)
    p = s.points(np.array([[0, 0, 0], [31, 0, 0], [0, 31, 0], [31, 31, 0], [0, 0, 31], [31, 0, 31]]) * U)
    t, u, z, r = p[0], p[1], p[2], p[3:]
    s.node([s.mask(np.concatenate([[t, u], r]), 0), s.mask(r, 1)], [1, 1, 1, 0], p)
    pfm = np.zeros((s.n, 4), bool)
    pfm[[t, *r], 0:2] = True
    pfm[[u, z], 3] = True
    return s.case(pfm, thr, t=int(t), u=int(u), z=int(z))


def _edge_merge(ni, nj, inter):
    """two nodes, a cluster each, all points kept: kept sets of ni and nj points sharing `inter`"""
    s = _Scene(2)
    g = np.stack(np.meshgrid(np.arange(3), np.arange(3), np.arange(3), indexing="ij"), axis=-1).reshape(-1, 3) * (15 * U)
    p = s.points(g[:ni + nj - inter])
    a, b = p[:ni], np.concatenate([p[:inter], p[ni:]])
    for pts in (a, b):
        s.node([s.mask(pts, 0), s.mask(pts, 1)], None, pts)
    return _all_seen(s, sets=(a, b))


def _edge_box(apart):
    """object i ends at x = 1 where object j begins: 5 shared points in that plane, one more on either side, so the
    boxes share a face, count as overlapping, and i merges into j (5 / 6).  apart: j's points are one double to the
    right of the plane instead (not dyadic), the boxes are disjoint and so are the sets."""
    s = _Scene(2)
    yz = np.array([[0, 0], [15, 0], [0, 15], [15, 15], [30, 0]]) * U
    plane = s.points(np.column_stack([np.full(5, 1.0), yz]))
    left = s.points(np.array([[1.0 - 15 * U, 0, 0]]))
    right = s.points(np.array([[1.0 + 15 * U, 0, 0]]))
    plane_j = s.points(np.column_stack([np.full(5, np.nextafter(1.0, 2.0)), yz])) if apart else plane
    for pts in (np.concatenate([plane, left]), np.concatenate([plane_j, right])):
        s.node([s.mask(pts, 0), s.mask(pts, 1)], None, pts)
    return _all_seen(s)


REPRE_TOP = [3, 66, 68, 10, 65]                                       # 5 / 8 at 3, 66, 68; 4 / 8 at 10, 65, 69


def _edge_repre():
    """an object of 8 points with 70 masks whose equal largest coverages sit in the first 64 list positions and
    past them; an object with 3 masks"""
    s = _Scene(8)
    cube = np.stack(np.meshgrid([0, 20], [0, 20], [0, 20], indexing="ij"), axis=-1).reshape(-1, 3) * U
    p = s.points(cube)
    n = {3: 5, 66: 5, 68: 5, 10: 4, 65: 4, 69: 4}
    s.node([s.mask(np.roll(p, -i)[:n.get(i, 2)], i % 8) for i in range(70)], None, p)
    q = s.points(cube + np.array([3.0, 0, 0]))
    s.node([s.mask(q[:6], 0), s.mask(q[2:], 1), s.mask(q, 2)], None, q)
    return _all_seen(s)


EDGE_CASES = {
    "eps_at": lambda: _edge_eps(False), "eps_below": lambda: _edge_eps(True),
    "border_y_first": lambda: _edge_border(False), "border_x_first": lambda: _edge_border(True),
    "noise_last": lambda: _edge_noise(True), "noise_none": lambda: _edge_noise(False), "no_core": _edge_no_core,
    "ratio_at": lambda: _edge_ratio(RATIO_EQ), "ratio_below": lambda: _edge_ratio(np.nextafter(RATIO_EQ, 0)),
    "ratio_negative": lambda: _edge_ratio(-1.0),
    "merge_4_of_5": lambda: _edge_merge(5, 10, 4), "merge_5_of_6": lambda: _edge_merge(6, 10, 5),
    "merge_j": lambda: _edge_merge(10, 6, 5), "merge_both": lambda: _edge_merge(6, 6, 5),
    "box_face": lambda: _edge_box(False), "box_apart": lambda: _edge_box(True),
    "repre": _edge_repre,
}
# neighbouring variants: the two sides of one rule, whose results must differ
EDGE_PAIRS = [("eps_at", "eps_below"), ("border_y_first", "border_x_first"), ("noise_last", "noise_none"),
              ("ratio_at", "ratio_below"), ("ratio_below", "ratio_negative"), ("merge_4_of_5", "merge_5_of_6"),
              ("merge_5_of_6", "merge_j"), ("merge_j", "merge_both"), ("box_face", "box_apart")]

SHIFT = (2.0 ** 17, -2.0 ** 16, 2.0 ** 15)
CASES = {
    "f65": lambda: _f_case(65), "f128": lambda: _f_case(128), "f129": lambda: _f_case(129), "f200": lambda: _f_case(200),
    "shifted": lambda: _f_case(65, SHIFT),
    "obj257": lambda: _obj_case(constants()["kPPBoxChunk"] + 1),
    "obj1025": lambda: _obj_case(constants()["kPPObjChunk"] + 1),
    "obj2049": lambda: _obj_case(2 * constants()["kPPObjChunk"] + 1),
    "n8192": lambda: _n_case(constants()["kPPLdsUF"]), "n8193": lambda: _n_case(constants()["kPPLdsUF"] + 1),
    "slots17": lambda: _slots_case(constants()["kPPSlots"] + 1), "slots40": lambda: _slots_case(40),
    "wide": lambda: _wide_case(2 ** 21 - 2),
}
CASES.update({"edges/" + k: v for k, v in EDGE_CASES.items()})
WIDE_REFUSED = lambda: _wide_case(2 ** 21 - 1)  # noqa: E731
DYADIC = [n for n in CASES if n not in ("edges/eps_at", "edges/eps_below", "edges/box_apart")]


@functools.lru_cache(maxsize=None)
def built(name) -> Case:
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(points, masks, details) of pp_oracle.post_process_objects on a case: computed once, left unchanged"""
    c = built(name)
    return pp_oracle.post_process_objects(*c.inputs, c.thr, eps=EPS, min_points=MIN_POINTS, overlapping_ratio=RATIO,
                                          details=True)


def expected_results(name):
    """the arrays of mc_pp_get_results as the oracle's details give them: every DBSCAN object of every node, kept
    or not, and every mask's choice"""
    c = built(name)
    wp, wm, det = oracle(name)
    nodes = [n for n in c.onodes if len(n[0]) >= 2]
    recs = det["nodes"]
    assert len(recs) == len(nodes)
    base = np.concatenate([[0], np.cumsum([len(r["objs"]) for r in recs])]).astype(np.int64)
    K = int(base[-1])
    state = np.zeros(K, np.uint8)
    for (ri, i), inv in zip(det["pre_obj"], det["invalid"]):
        state[base[ri] + i] = 1 if inv else 2
    ent, mobj, mcov, box = [], [], [], np.zeros((K, 6))
    for ri, r in enumerate(recs):
        e = np.full(len(r["lab"]), -1, np.int32)
        for i, (o, v) in enumerate(zip(r["objs"], r["valid"])):
            if state[base[ri] + i] == 2:
                e[o[v]] = base[ri] + i
            box[base[ri] + i] = np.concatenate(r["box"][i])
        ent.append(e)
        mobj += [base[ri] + b if b >= 0 else -1 for b, _ in r["mask_best"]]
        mcov += [cov for _, cov in r["mask_best"]]
    return dict(entry_object=np.concatenate(ent) if ent else np.zeros(0, np.int32), mask_object=np.asarray(mobj, np.int32),
                mask_coverage=np.asarray(mcov, np.float64), object_state=state,
                object_node=np.repeat(np.arange(len(recs)), np.diff(base)).astype(np.int32), object_bbox=box,
                info=(K, len(det["pre_obj"]), len(wp), sum(len(n[2]) for n in nodes), sum(len(n[0]) for n in nodes)))


def frame_reach(name):
    """what an f case reaches, from its inputs and the oracle: FW, the nodes' W, the masks' frame ranks, the points
    seen in no visible frame of their node, the points kept and dropped by the ratio, the final objects"""
    c = built(name)
    wp, _, det = oracle(name)
    F = c.pfm.shape[1]
    W, fp, blind = [], set(), 0
    for masks, vf, order in c.onodes:
        vcols = np.nonzero(vf)[0]
        W.append((len(vcols) + 63) // 64)
        fp |= {int(np.searchsorted(vcols, c.mask_col[m])) for m in masks}
        blind += int((c.pfm[order][:, vcols].sum(1) == 0).sum())
    valid = np.concatenate([v for r in det["nodes"] for v in r["valid"]])
    return dict(FW=(F + 63) // 64, W=set(W), fp=fp, blind=blind, kept=int(valid.sum()), dropped=int((~valid).sum()),
                final=len(wp))


def most_objects_on_a_point(name):
    """the largest number of kept objects (before the merge) that hold one point as a kept point: k_pp_index's count"""
    _, _, det = oracle(name)
    return int(np.bincount(np.concatenate(det["pre_pts"])).max())
