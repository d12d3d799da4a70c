"""Inputs that put S1's pixel stage (mc_bp_pixels.inl) and voxel stage (mc_bp_voxel.inl) on every size-dependent
branch, and what each must reach.  numpy and the oracle only: test_s1_voxel_inputs_cpu.py asserts without a GPU
that every case reaches what it is for; test_gpu_s1_voxel.py reads the device's pixel lists and voxel means back
(Context.bp_voxels) and compares them bit for bit.

restate() is a numpy restatement of a slot's valid pixels, world points, grid origin, voxel indices and voxel
numbers (first occurrence), independent of oracle/s1_oracle.c; the means are oracle.s1_voxel of its world points
(the sequential fold).  abandons() is a model of one k_bp_voxel_lds tier: which of its three ways of handing a
slot on it takes, if any.  The tiers' sizes are read out of mc_bp_voxel.inl (constants()), never retyped.

  case                 input                                                      reaches
  v511 .. v8193        the row-major prefix of m pixels of a tilted noisy          the voxel counts on both sides of
                       surface under a generic rigid pose, ~2.6 pixels per         kVxL2, kVxV, kVxH and kVxV2; the
                       voxel, a voxel's pixels a row (= most of a chunk) apart;    overflowing voxel is the slot's
                       m the largest with the count / the smallest with one more   last pixel
  table                near rows, then three rows at ~6 m (a voxel per pixel)      tier 1's hash table fills before
                                                                                   the id test sees it; tier 2 keeps
  span1023, span1024   identity pose, a row at depth 1.0 and one at 11.232 /       largest z index 1023 (kept) / 1024
                       11.238                                                      (both tiers hand on: k_bp_voxel)
  runs                 depth ~0.04 m: 16 voxels of thousands of pixels             runs of equal keys over whole waves
                                                                                   and across lane 0; the fold's order
  chunks               slots of exactly 25, 256, 257, 512, 513 pixels              the prefetch clamps of both tiers
  pix96, pix98         100 rows, 96 / 98 wide, two frames: ids 1 + (u + 3 v) % 255  vec4 and scalar loads; a partial last
                       (about 102 ids in a wave's 256-pixel step) and ids           band; in the second frame all 255
                       1 + (u + W v) % 255; an id of 24 and one of 25 valid         ids in every step
                       pixels; depth 0, NaN, negative, inf, > trunc under ids
  idx21ok, idx21over   voxel_size 2^-18, identity pose, depths 1.0 and             largest index 2^21 - 1 (accepted) /
                       9 - 2^-18 / 9.0                                             2^21 (MC_ERR_UNSUPPORTED)
"""
import functools
import os
import re
from typing import NamedTuple

import numpy as np

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskclustering_amd", "csrc")
SPAN = 1024            # voxel indices per axis of an LDS tier's 30-bit key (k_bp_voxel_lds: r < 1024.0)
AXIS_LIMIT = 1 << 21   # voxel indices per axis of k_bp_voxel's key
FEW, TRUNC, VOXEL = 25, 20.0, 0.01
MARGIN = 1e-9          # s1_witness.MARGIN_F64
H_MAX, W_MAX = 200, 208
COUNTS = (511, 512, 513, 2048, 2049, 2177, 8192, 8193)
CHUNK_SIZES = (25, 256, 257, 512, 513)


@functools.lru_cache(maxsize=None)
def constants():
    """the tiers' sizes and the band height, read out of the sources"""
    with open(os.path.join(CSRC, "mc_bp_voxel.inl")) as f:
        vox = f.read()
    with open(os.path.join(CSRC, "mc_bp_kernels.inl")) as f:
        kern = f.read()
    c = {}
    for n in ("kVxT", "kVxH", "kVxV", "kVxT2", "kVxH2", "kVxV2", "kVxL2"):
        m = re.findall(r"^constexpr int [^\n]*\b%s = (\d+)[,;]" % n, vox, re.M)
        assert len(m) == 1, (n, m)
        c[n] = int(m[0])
    m = re.findall(r"constexpr int kBpBand = (\d+);", kern)
    assert len(m) == 1
    c["kBpBand"] = int(m[0])
    assert "r < 1024.0" in vox and "(1ll << 21)" in vox      # SPAN, AXIS_LIMIT
    return c


def tiers():
    """((T, H, V) of the first tier, of the second)"""
    c = constants()
    return (c["kVxT"], c["kVxH"], c["kVxV"]), (c["kVxT2"], c["kVxH2"], c["kVxV2"])


# ---- the restatement ----
class Slot(NamedTuple):
    pixels: np.ndarray   # u32 [n]: v * W + u of the valid pixels, row-major
    world: np.ndarray    # f64 [n, 3]
    vmin: np.ndarray     # f64 [3]: the grid origin
    t: np.ndarray        # f64 [n, 3]: (p - vmin) / voxel
    index: np.ndarray    # i64 [n, 3]: floor(t)
    rank: np.ndarray     # i64 [n]: the pixel's voxel number (voxels in order of their first pixel)
    nvox: int


def world_of(pix, depth, K, T):
    """world points of the pixels pix (v * W + u) of one frame: ((u - cx) z / fx, (v - cy) z / fy, z), then
    ((T0 x + T1 y) + T2 z) + T3 per row of the pose and the divide by row 3"""
    depth = np.asarray(depth, np.float32)
    W = depth.shape[1]
    fx, fy, cx, cy = np.asarray(K, np.float64).reshape(4)
    T = np.asarray(T, np.float64).reshape(4, 4)
    v, u = np.divmod(np.asarray(pix, np.int64), W)
    z = depth.reshape(-1)[pix].astype(np.float64)
    x = (u.astype(np.float64) - cx) * z / fx
    y = (v.astype(np.float64) - cy) * z / fy
    r = [((T[k, 0] * x + T[k, 1] * y) + T[k, 2] * z) + T[k, 3] for k in range(4)]
    return np.stack([r[0] / r[3], r[1] / r[3], r[2] / r[3]], axis=1)


def first_rank(index):
    """voxel numbers by first occurrence of the rows of index [n, 3] (non-negative, < 2^21 + 1 per axis)"""
    key = (index[:, 0] << 44) | (index[:, 1] << 22) | index[:, 2]
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    number = np.empty(len(first), np.int64)
    number[np.argsort(first, kind="stable")] = np.arange(len(first))
    return number[inv.reshape(-1)]


def restate(depth, seg, K, T, mask_id, trunc=TRUNC, voxel=VOXEL):
    depth = np.asarray(depth, np.float32)
    with np.errstate(invalid="ignore"):
        ok = (np.asarray(seg) == mask_id) & (depth > 0) & (depth.astype(np.float64) < trunc)
    pix = np.flatnonzero(ok)
    p = world_of(pix, depth, K, T)
    vmin = p.min(axis=0) - voxel * 0.5
    t = (p - vmin) / voxel
    index = np.floor(t).astype(np.int64)
    rank = first_rank(index)
    return Slot(pix.astype(np.uint32), p, vmin, t, index, rank, int(rank.max()) + 1 if len(rank) else 0)


def restate_frame(depth, seg, K, T, trunc=TRUNC, voxel=VOXEL, few=FEW):
    """{id: Slot} of the frame's candidate slots (ids with at least few valid pixels), ids ascending"""
    out = {}
    for i in np.unique(seg):
        if i == 0:
            continue
        s = restate(depth, seg, K, T, int(i), trunc, voxel)
        if len(s.pixels) >= few:
            out[int(i)] = s
    return out


# ---- the model of a tier ----
def abandons(rank, index, T, H, V):
    """how k_bp_voxel_lds<T, H, V> hands the slot on: chunks of T pixels in list order; 'span' when a chunk has
    an index >= 1024, 'table' when after a chunk the distinct keys exceed the H hash entries (a probe finds no
    entry) while before it they did not exceed V, 'ids' when they exceed V; None: the tier keeps the slot"""
    seen = np.maximum.accumulate(rank) + 1        # distinct keys among the first k + 1 pixels
    for c0 in range(0, len(rank), T):
        c1 = min(c0 + T, len(rank))
        if (index[c0:c1] >= SPAN).any():
            return "span"
        if seen[c1 - 1] > H:
            return "table"
        if seen[c1 - 1] > V:
            return "ids"
    return None


def route(slot):
    """(the first tier's verdict, the second's or None where the first keeps)"""
    t1, t2 = tiers()
    a = abandons(slot.rank, slot.index, *t1)
    return a, (abandons(slot.rank, slot.index, *t2) if a else None)


def handed(slots):
    """(slots the first tier hands on, slots the second hands on) of these slots"""
    r = [route(s) for s in slots]
    return sum(1 for a, _ in r if a), sum(1 for a, b in r if a and b)


# ---- frames ----
class Case(NamedTuple):
    depth: np.ndarray    # f32 [F, H, W]
    seg: np.ndarray      # u8 [F, H, W]
    K: np.ndarray        # f64 [F, 4]
    T: np.ndarray        # f64 [F, 4, 4]
    voxel: float
    want: dict           # what the case is for (check_case)

    def scene(self, step=2):
        """float32 scene points: every step-th valid pixel's own world point, so that masks survive the query"""
        pts = []
        for f in range(len(self.depth)):
            with np.errstate(invalid="ignore"):
                ok = (self.depth[f] > 0) & (self.depth[f].astype(np.float64) < TRUNC)
            pts.append(world_of(np.flatnonzero(ok)[::step], self.depth[f], self.K[f], self.T[f]))
        return np.concatenate(pts).astype(np.float32)

    def slots(self, f=0):
        return restate_frame(self.depth[f], self.seg[f], self.K[f], self.T[f], voxel=self.voxel)


def _case(depth, seg, K, T, voxel=VOXEL, **want):
    depth = np.ascontiguousarray(depth, np.float32)
    seg = np.ascontiguousarray(seg, np.uint8)
    F = len(depth)
    out = Case(depth, seg, np.ascontiguousarray(np.broadcast_to(np.asarray(K, np.float64), (F, 4))),
               np.ascontiguousarray(np.broadcast_to(np.asarray(T, np.float64), (F, 4, 4))), float(voxel), want)
    for a in out[:4]:
        a.setflags(write=False)
    return out


def generic_pose():
    """a rigid pose with no axis of the camera along an axis of the world"""
    a = np.array([0.50, 0.62, 0.60])
    b = np.array([0.70, -0.60, 0.10])
    a /= np.linalg.norm(a)
    b -= a * (a @ b)
    b /= np.linalg.norm(b)
    T = np.eye(4)
    T[:3, 0], T[:3, 1], T[:3, 2] = b, a, np.cross(b, a)
    T[:3, 3] = [0.37, -1.21, 0.83]
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12 and np.abs(T[:3, :3]).min() > 0.05
    return T


SURFACE_K = np.array([190.0, 640.0, 104.3, 99.8])   # a column apart is about a voxel, a row about a third


def surface(H=H_MAX, W=W_MAX, z0=2.0, seed=11, noise=2e-4, K=SURFACE_K):
    """depths of a smooth tilted surface plus noise"""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:H, 0:W].astype(np.float64)
    z = z0 * (1.0 + 0.11 * (u - K[2]) / W + 0.07 * (v - K[3]) / H + 0.02 * np.sin(u / 37.0) * np.cos(v / 29.0))
    return (z + rng.uniform(-noise, noise, size=z.shape)).astype(np.float32)


def prefix_seg(H, W, m, mask_id=1):
    seg = np.zeros(H * W, np.uint8)
    seg[:m] = mask_id
    return seg.reshape(H, W)


@functools.lru_cache(maxsize=None)
def _surface_counts():
    """(depth, pose, nvox of the prefix of m pixels for the m it was asked for) of the surface frame"""
    depth, T = surface(), generic_pose()
    memo = {}

    def nvox(m):
        if m not in memo:
            memo[m] = restate(depth, prefix_seg(H_MAX, W_MAX, m), SURFACE_K, T, 1).nvox
        return memo[m]
    return depth, T, nvox


def prefix_for(count):
    """the largest m with nvox(m) == count (the next pixel opens voxel count + 1), found from a bisection of
    the near-monotone count; the count is asserted by the caller against the oracle"""
    depth, T, nvox = _surface_counts()
    lo, hi = FEW, H_MAX * W_MAX
    assert nvox(hi) > count, "the surface frame has too few voxels"
    while hi - lo > 1:                     # nvox(lo) <= count < nvox(hi)
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if nvox(mid) <= count else (lo, mid)
    assert nvox(lo) == count and nvox(lo + 1) == count + 1, (count, lo, nvox(lo), nvox(lo + 1))
    return lo


def count_case(count):
    """the prefix with exactly count voxels: the largest for a count on the keeping side of a limit, the smallest
    for one more (its last pixel then opens the last voxel)"""
    c = constants()
    keeping = count in (c["kVxL2"] - 1, c["kVxL2"], c["kVxV"], c["kVxV2"])
    depth, T, _ = _surface_counts()
    m = prefix_for(count) if keeping else prefix_for(count - 1) + 1
    return _case(depth[None], prefix_seg(H_MAX, W_MAX, m)[None], SURFACE_K, T, nvox={1: count}, last_opens=not keeping)


def table_case():
    """r near rows of the surface, then three rows at ~6 m where every pixel is its own voxel: the r whose count
    at some chunk start is at most kVxV and more than kVxH a chunk later, found with the model"""
    (t1, h1, v1), _ = tiers()
    T = generic_pose()
    near = surface()
    far = surface(z0=6.0, seed=12)
    for r in range(8, 60):
        depth = near.copy()
        depth[r:r + 3] = far[r:r + 3]
        c = _case(depth[None], prefix_seg(H_MAX, W_MAX, (r + 3) * W_MAX)[None], SURFACE_K, T)
        s = c.slots()[1]
        if route(s) == ("table", None):
            nn = int(s.rank[:r * W_MAX].max()) + 1
            return c._replace(want=dict(nvox={1: s.nvox}, route={1: ("table", None)}, near=nn, far=s.nvox - nn))
    raise AssertionError("no number of near rows takes the first tier's table route")


def span_case(far):
    W = W_MAX
    depth = np.zeros((2, W), np.float32)
    depth[0], depth[1] = 1.0, far
    K = [300.0, 300.0, W / 2 + 0.3, 0.6]
    return _case(depth[None], prefix_seg(2, W, 2 * W)[None], K, np.eye(4))


def runs_case():
    """depth ~0.04 m: a pixel is about a fiftieth of a voxel wide"""
    T = generic_pose()
    T[:3, 3] = 0.0
    depth = surface(z0=0.04, seed=13, noise=2e-7)
    return _case(depth[None], prefix_seg(H_MAX, W_MAX, 23000)[None], SURFACE_K, T)


def chunks_case():
    depth = surface()
    seg = np.zeros(H_MAX * W_MAX, np.uint8)
    o = 0
    for i, n in enumerate(CHUNK_SIZES):
        seg[o:o + n] = i + 1
        o += n
    return _case(depth[None], seg.reshape(1, H_MAX, W_MAX), SURFACE_K, generic_pose(),
                 npix={i + 1: n for i, n in enumerate(CHUNK_SIZES)})


PIX_SHORT, PIX_EXACT = 7, 8     # the ids cut down to FEW - 1 and to FEW valid pixels


def pixels_case(W, H=100):
    """every id in every wave's step; invalid depths of each kind under ids; an id just under and one on few_points"""
    K = np.array([190.0, 640.0, W / 2 + 0.3, H / 2 - 0.2])
    v, u = np.mgrid[0:H, 0:W]
    # frame 0: a row's ids ascend and the next row starts three on; frame 1: the ids ascend through the frame,
    # so that any 255 consecutive pixels (a wave's step is 256) hold every id
    segs = [(1 + (u + 3 * v) % 255).astype(np.uint8), (1 + (u + W * v) % 255).astype(np.uint8)]
    depths = []
    for f, seg in enumerate(segs):
        depth = surface(H, W, seed=14 + f, K=K).copy()
        flat, ids = depth.reshape(-1), seg.reshape(-1)
        for i, keep in ((PIX_SHORT, FEW - 1), (PIX_EXACT, FEW)):
            at = np.flatnonzero(ids == i)
            assert len(at) > keep + 3
            cut = at[keep // 2:keep // 2 + len(at) - keep]          # from the middle of the id's list
            flat[cut] = np.resize(np.array([0.0, np.nan, 25.0, -1.0], np.float32), len(cut))
        other = np.flatnonzero((ids != PIX_SHORT) & (ids != PIX_EXACT))[5::97]
        flat[other] = np.resize(np.array([np.nan, 0.0, 20.5, np.inf], np.float32), len(other))
        assert not (flat.astype(np.float64) == TRUNC).any()
        depths.append(depth)
    return _case(np.stack(depths), np.stack(segs), K, generic_pose(), short=PIX_SHORT, exact=PIX_EXACT)


def index21_case(over):
    """voxel_size 2^-18: z indices 0 and 2^21 - 1 (depth 9 - 2^-18) or 2^21 (depth 9.0), (p - vmin) / voxel = k + 0.5"""
    W = 32
    depth = np.full((1, W), 1.0, np.float32)
    depth[0, W - 1] = 9.0 if over else 9.0 - 2.0 ** -18
    assert float(depth[0, W - 1]) == (9.0 if over else 9.0 - 2.0 ** -18)
    K = [301.7, 299.3, W / 2 + 0.3, 0.4]
    return _case(depth[None], prefix_seg(1, W, W)[None], K, np.eye(4), voxel=2.0 ** -18, over=bool(over))


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("v") and name[1:].isdigit():
        return count_case(int(name[1:]))
    if name == "table":
        return table_case()
    if name in ("span1023", "span1024"):
        return span_case(11.232 if name == "span1023" else 11.238)
    if name == "runs":
        return runs_case()
    if name == "chunks":
        return chunks_case()
    if name in ("pix96", "pix98"):
        return pixels_case(int(name[3:]))
    if name in ("idx21ok", "idx21over"):
        return index21_case(name == "idx21over")
    raise KeyError(name)


COUNT_CASES = ["v%d" % c for c in COUNTS]
L2_CASES = COUNT_CASES[:3]                       # also with every slot forced to the second tier: the kVxL2 edge
CASES = COUNT_CASES + ["table", "span1023", "span1024", "runs", "chunks", "pix96", "pix98", "idx21ok"]

# the tiers' verdicts the cases are for (route())
ROUTES = {"v511": (None, None), "v512": (None, None), "v513": (None, None), "v2048": (None, None),
          "v2049": ("ids", None), "v2177": ("ids", None), "v8192": ("ids", None), "v8193": ("ids", "ids"),
          "table": ("table", None), "span1023": (None, None), "span1024": ("span", "span"), "runs": (None, None),
          "idx21ok": ("span", "span"), "idx21over": ("span", "span")}


def oracle_frame(c, f=0):
    """the oracle's (labels, off, pts, stats) of frame f of the case, with the case's own scene points"""
    from oracle import oracle
    prm = oracle.BpParams.default(voxel_size=c.voxel)
    return oracle.s1_frame(c.scene(), c.depth[f], c.seg[f], c.K[f], c.T[f], prm)


def oracle_means(slot, voxel=VOXEL):
    from oracle import oracle
    return oracle.s1_voxel(slot.world, voxel)


def longest_runs(rank):
    """(the longest run of equal consecutive voxel numbers, whether a run covers a whole aligned 64-pixel wave,
    whether a run continues from a wave's last lane into the next wave's lane 0)"""
    change = np.flatnonzero(np.diff(rank) != 0) + 1
    start = np.concatenate([[0], change])
    end = np.concatenate([change, [len(rank)]])
    whole = any(-(-a // 64) * 64 + 64 <= b for a, b in zip(start, end))
    cross = any(a < 64 * k <= b - 1 for a, b in zip(start, end) for k in range(a // 64 + 1, b // 64 + 1))
    return int((end - start).max()), whole, cross


def check_case(name):
    """the conditions of one case, from the restatement, the model and the oracle; returns a report"""
    import s1_witness as W
    c = case(name)
    const = constants()
    assert c.depth.shape[1] <= H_MAX and c.depth.shape[2] <= W_MAX
    rep = dict(routes={})
    for f in range(len(c.depth)):
        slots = c.slots(f)
        ost = oracle_frame(c, f)[3]
        want_nvox = {int(r[0]): int(r[2]) for r in ost if r[1] >= FEW}
        assert {i: s.nvox for i, s in slots.items()} == want_nvox, f"{name}: voxel counts differ from the oracle's"
        rep["npix"] = {i: len(s.pixels) for i, s in slots.items()} if len(slots) < 8 else len(slots)
        for i, s in slots.items():
            assert len(s.pixels) <= 23100
            assert s.index.min() >= 0
            edge = float(np.abs(s.t - np.rint(s.t)).min())
            assert edge > MARGIN, f"{name} id {i}: (p - vmin) / voxel within {edge} of an integer"
            means = oracle_means(s, c.voxel)
            assert len(means) == s.nvox
            wm, wv, _ = W.voxel_means(s.world, c.voxel)
            np.testing.assert_array_equal(wv, s.rank)
            cnt = np.bincount(s.rank)
            err = np.abs(means - wm.astype(np.float64))
            assert (err <= (cnt * 2.0 ** -52 * np.abs(means).max())[:, None]).all(), f"{name} id {i}: {err.max()}"
            rep["routes"][f, i] = route(s)
        if name.startswith("pix"):
            H, Wd = c.depth.shape[1:]
            assert H % const["kBpBand"] != 0 and (Wd % 4 == 0) == (name == "pix96")
            ids = c.seg[f].reshape(-1)
            if f == 1:
                assert all(len(np.unique(ids[k:k + 256])) == 255 for k in range(0, H * Wd - 255, 64))
            assert c.want["short"] not in slots and len(slots[c.want["exact"]].pixels) == FEW
            npix = {int(r[0]): int(r[1]) for r in ost}
            assert npix[c.want["short"]] == FEW - 1
            d = c.depth[f]
            assert np.isnan(d).any() and (d == 0).any() and (d > TRUNC).any() and len(slots) == 254
    if len(rep["routes"]) < 8:
        rep["routes"] = {i: r for (_, i), r in rep["routes"].items()}
    else:
        assert set(rep["routes"].values()) == {(None, None)}
        rep["routes"] = len(rep["routes"])
    if name in ROUTES:
        assert rep["routes"] == {1: ROUTES[name]}, (name, rep["routes"])
    if "nvox" in c.want:
        assert {i: s.nvox for i, s in slots.items()} == c.want["nvox"]
    if c.want.get("last_opens"):
        s = slots[1]
        assert s.rank[-1] == s.nvox - 1 and (s.rank[:-1] < s.nvox - 1).all(), "the last voxel is not the last pixel's"
    if name in COUNT_CASES:
        s = slots[1]
        per = np.bincount(s.rank)
        gap = np.concatenate([np.diff(np.flatnonzero(s.rank == v)) for v in range(0, s.nvox, 37) if per[v] > 1])
        rep["pixels_per_voxel"] = len(s.rank) / s.nvox
        rep["continued"] = float((gap > const["kVxT"] // 2).mean())
        assert 1.8 < rep["pixels_per_voxel"] < 3.5 and rep["continued"] > 0.5    # sums continue across chunks
    if name == "table":
        (t1, h1, v1), _ = tiers()
        assert c.want["near"] <= v1 and c.want["near"] + c.want["far"] > h1
        rep.update(near=c.want["near"], far=c.want["far"])
    if name.startswith("span"):
        assert int(slots[1].index.max()) == int(name[4:]) and int(slots[1].index[:, :2].max()) < SPAN - 1
    if name == "runs":
        s = slots[1]
        rep["runs"] = longest_runs(s.rank)
        rep["nvox"], rep["largest"] = s.nvox, int(np.bincount(s.rank).max())
        assert rep["runs"][1] and rep["runs"][2] and rep["largest"] > 4 * const["kVxT2"]
        means = oracle_means(s)
        # numpy's own order: pairwise over a contiguous axis
        pair = np.stack([np.ascontiguousarray(s.world[s.rank == v].T).sum(axis=1) / (s.rank == v).sum() for v in range(s.nvox)])
        rep["order_changes"] = int((pair.view(np.uint64) != means.view(np.uint64)).any(axis=1).sum())
        assert rep["order_changes"] >= 1, "summation order does not show in this case's means"
    if name == "chunks":
        assert {i: len(s.pixels) for i, s in slots.items()} == c.want["npix"]
    if name.startswith("idx21"):
        s = slots[1]
        assert int(s.index[:, 2].max()) == (AXIS_LIMIT if c.want["over"] else AXIS_LIMIT - 1)
        assert int(s.index[:, :2].max()) < AXIS_LIMIT - 1
        fr = s.t[:, 2] - np.floor(s.t[:, 2])
        assert (fr == 0.5).all()
    return rep
