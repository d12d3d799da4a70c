"""The inputs of test_gpu_pp_limits.py, checked without a GPU (pp_limit_inputs.py): the constants are read out of
the sources, every case reaches the branch it is meant to pin (asserted from its inputs and from the oracle's
result on it), the two sides of every rule give different results, and on every case whose coordinates keep each
pair away from eps the oracle's DBSCAN equals scikit-learn's (core points' partition and noise set): the
independent witness for the large cases, which the reference's own golden does not reach.

Measured: the whole file takes 17.5 s on one CPU core, 16.5 s of it the oracle, once per case (obj2049 8.5 s,
obj1025 2.8 s, n8192 and n8193 2.2 s each); the pair margins and scikit-learn take under a second together."""
import numpy as np
import pytest

import pp_limit_inputs as pl

K = pl.constants()
# Dyadic coordinates: d^2 is an integer number of U^2 and eps^2 is 10485.76 U^2, so |d^2 - eps^2| >= 0.24 U^2 and
# |d - eps| >= 0.24 U^2 / (2 * 102.4 U) > 1.1e-3 U = 1.1e-6 m, ten orders above the rounding of a float64 distance.
MARGIN = 1e-6


def _same(a, b):
    (ap, am), (bp, bm) = a[:2], b[:2]
    return len(ap) == len(bp) and all(np.array_equal(x, y) for x, y in zip(ap, bp)) and am == bm


def test_constants_are_read_from_the_sources():
    assert all(isinstance(v, int) and v > 0 for v in K.values()) and len(K) == 7
    assert K["kPPBoxChunk"] < K["kPPObjChunk"] and K["kPPObjChunk"] % 64 == 0      # the tie cases' lanes and windows
    assert K["dbscan_threads"] == K["kPPItemPoints"]            # n8192's small nodes sit on both at once
    assert K["kPPMaxKept"] ** 2 < 2 ** 31 <= (K["kPPMaxKept"] + 1) ** 2            # stated only: 46 341 kept objects
    assert 4 * (2 * K["kPPObjChunk"] + 1) > K["kPPLdsUF"]       # obj2049's nodes also take the split DBSCAN


@pytest.mark.parametrize("name,F,FW,W,fps", [("f65", 65, 2, {1, 2}, {0, 62, 63, 64}), ("f128", 128, 2, {1, 2}, {0, 62, 63, 64}),
                                             ("f129", 129, 3, {1, 2, 3}, {0, 63, 64, 127, 128}),
                                             ("f200", 200, 4, {1, 2, 3}, {0, 63, 64, 127, 128}), ("shifted", 65, 2, {1, 2}, {63, 64})])
def test_frame_cases(name, F, FW, W, fps):
    c, r = pl.built(name), pl.frame_reach(name)
    assert c.pfm.shape[1] == F and r["FW"] == FW and r["W"] == W and fps <= r["fp"]
    assert r["blind"] > 0 and r["kept"] > 0 and r["dropped"] > 0 and r["final"] >= 1
    words = [c.pfm[:, 64 * w:64 * w + 64].any(1) for w in range(FW)]
    assert all(w.mean() > 0.8 for w in words)                    # bits in every word (the blind points excepted)
    nvs = sorted(int(n[1].sum()) for n in c.onodes)
    assert nvs == [1, 63, 64, 65] + ([129] if F >= 129 else [])
    seen_cols = set()
    for masks, vf, order in c.onodes:
        vcols, cols = np.nonzero(vf)[0], {int(c.mask_col[m]) for m in masks}
        seen_cols |= cols
        assert vcols[0] in cols and vcols[-1] in cols and len(order) >= 180
        for rank in (63, 64, 127, 128):                         # a mask on each side of every word edge of the ranks
            assert rank >= len(vcols) or vcols[rank] in cols
        for col in (63, 64, 127, 128):                          # and of the columns
            assert not (col < F and vf[col]) or col in cols
    assert {col for col in (0, 63, 64, 127, 128, F - 1) if col < F} <= seen_cols


def test_shifted_scene_has_the_same_result():
    a, b = pl.built("f65"), pl.built("shifted")
    np.testing.assert_array_equal(b.scene - np.asarray(pl.SHIFT), a.scene)         # the shift is exact
    assert np.abs(b.scene).min() >= 2.0 ** 15 - 8
    assert _same(pl.oracle("f65"), pl.oracle("shifted"))


@pytest.mark.parametrize("name", ["obj257", "obj1025", "obj2049"])
def test_object_window_cases(name):
    c, (wp, wm, det) = pl.built(name), pl.oracle(name)
    C, box, chunk = c.meta["clusters"], K["kPPBoxChunk"], K["kPPObjChunk"]
    nobj = [len(r["objs"]) for r in det["nodes"]]
    assert nobj == [C, C + 1]
    assert C == {"obj257": box + 1, "obj1025": chunk + 1, "obj2049": 2 * chunk + 1}[name]
    assert [int((r["lab"] == 0).sum()) for r in det["nodes"]] == [0, 1]            # nsh = 1 and 0
    q = 0
    for ri, r in enumerate(det["nodes"]):                         # every mask chooses the object it was built for
        for m, (best, cov) in zip(c.onodes[ri][0], r["mask_best"]):
            assert c.meta["want_best"][m] == (ri, best), (m, best)
            q += 1
    wanted = {w for _, w in c.meta["want_best"].values()}
    assert -1 in wanted and q == len(c.meta["want_best"])
    if C > chunk:
        assert {5, 7, 9, chunk} <= wanted                         # ties (a), (b); the later, larger count (c)
    if C > 2 * chunk:
        assert {6, 11, chunk + 7, chunk + 3, 2 * chunk} <= wanted
    for e in (box, chunk, 2 * chunk):                             # either side of every window edge the node has
        for ri, r in enumerate(det["nodes"]):
            if e >= nobj[ri]:
                continue
            kept = [int(r["valid"][o].sum()) for o in (e - 1, e)]
            assert all(0 < k < 4 for k in kept) and kept[0] != kept[1]
            assert not np.array_equal(r["box"][e - 1][0], r["box"][e][0])
            final = {(a, b) for (a, b), inv in zip(det["pre_obj"], det["invalid"]) if not inv}
            assert (ri, e - 1) in final and (ri, e) in final      # and both reach the export


@pytest.mark.parametrize("name", ["n8192", "n8193"])
def test_node_size_cases(name):
    c, (wp, wm, det) = pl.built(name), pl.oracle(name)
    uf, nt = K["kPPLdsUF"], K["dbscan_threads"]
    sizes = c.meta["sizes"]
    assert sizes == [uf + (name == "n8193"), nt - 1, nt, nt + 1]
    assert pl.big_items(sizes, uf) == ((0, 0) if name == "n8192" else (1, 17))     # the default big_min
    assert pl.big_items(sizes, uf + 1) == (0, 0)                  # MC_PP_BIG_MIN = kPPLdsUF + 1: k_pp_dbscan's global branch
    assert pl.big_items(sizes, 500) == (4, -(-sizes[0] // K["kPPItemPoints"]) + 1 + 1 + 2)
    big = det["nodes"][0]
    assert sorted(len(o) for o in big["objs"]) == [1, 4, 4, sizes[0] - 9]          # noise, two clusters, the lattice
    assert [len(r["objs"]) for r in det["nodes"][1:]] == [1, 1, 1]
    assert not np.array_equal(c.onodes[0][2], np.sort(c.onodes[0][2]))              # shuffled list order
    assert len(wp) >= 5


@pytest.mark.parametrize("name", ["slots17", "slots40"])
def test_slot_cases(name):
    c, (wp, wm, det) = pl.built(name), pl.oracle(name)
    m = c.meta["nodes"]
    assert pl.most_objects_on_a_point(name) == m > K["kPPSlots"]
    assert m == (K["kPPSlots"] + 1 if name == "slots17" else 40)
    dup = [inv for (ri, _), inv in zip(det["pre_obj"], det["invalid"]) if ri < m]
    assert len(dup) == m and 2 <= sum(not i for i in dup) < m     # near-duplicates: some merge, some stay


def test_wide_cases():
    ce = pl.EPS * 1.01
    ok, refused = pl.built("wide"), pl.WIDE_REFUSED()
    assert np.floor(np.ptp(ok.scene[:, 0]) / ce) == 2 ** 21 - 2 and np.floor(np.ptp(refused.scene[:, 0]) / ce) == 2 ** 21 - 1
    assert "static_cast<double>((1 << 21) - 1)" in pl._src("mc_pp_kernels.inl")
    assert "< kPPMaxCells))" in pl._src("mc_pp_layout.inl")        # k_pp_prep's test against it
    wp, wm, det = pl.oracle("wide")
    assert [len(p) for p in wp] == [4, 4]


def test_rule_edges_are_exact():
    x = np.nextafter(0.1, 0)
    assert not (0.1 * 0.1 < pl.EPS * pl.EPS) and x * x < pl.EPS * pl.EPS
    assert not (4 / 5 > pl.RATIO) and 5 / 6 > pl.RATIO
    assert not (1 / (2 + 1e-6) > pl.RATIO_EQ) and 1 / (2 + 1e-6) > np.nextafter(pl.RATIO_EQ, 0)
    assert 1 / (0 + 1e-6) > 1e5 and not (0 / (0 + 1e-6) > pl.RATIO_EQ) and 0 / (0 + 1e-6) > -1.0


@pytest.mark.parametrize("a,b", pl.EDGE_PAIRS)
def test_neighbouring_edge_variants_differ(a, b):
    assert not _same(pl.oracle("edges/" + a), pl.oracle("edges/" + b))


def test_edge_variants_decide_as_stated():
    pts = lambda n: [sorted(p.tolist()) for p in pl.oracle("edges/" + n)[0]]  # noqa: E731
    assert pts("eps_at") == [[0, 1, 2, 3, 4], [5, 6, 7, 8]] and pts("eps_below") == [[0, 1, 2, 3], [5, 6, 7, 8]]
    c = pl.built("edges/border_y_first")
    q, x, y = c.meta["q"], c.meta["x"].tolist(), c.meta["y"].tolist()
    assert c.onodes[0][2][0] == q
    assert pts("border_y_first") == [sorted(y + [q]), x] and pts("border_x_first") == [sorted(x + [q]), y]
    assert pts("noise_last") == [[4], [0, 1, 2, 3]] and pts("noise_none") == [[0, 1, 2, 3]]
    assert pts("no_core") == [[0, 1, 2], [3, 4, 5, 6]]
    labs = [r["lab"].tolist() for r in pl.oracle("edges/no_core")[2]["nodes"]]
    assert labs == [[0, 0, 0], [1, 1, 1, 1]]                      # all noise (class 0); one cluster and no noise
    m = pl.built("edges/ratio_at").meta
    every = set(range(6))
    assert set(pts("ratio_at")[0]) == every - {m["t"], m["z"]} and m["u"] in pts("ratio_at")[0]
    assert set(pts("ratio_below")[0]) == every - {m["z"]} and set(pts("ratio_negative")[0]) == every
    sets = lambda n: [sorted(s.tolist()) for s in pl.built("edges/" + n).meta["sets"]]  # noqa: E731
    assert pts("merge_4_of_5") == sets("merge_4_of_5")            # no merge
    assert pts("merge_5_of_6") == sets("merge_5_of_6")[1:] and pts("merge_j") == sets("merge_j")[:1]
    assert pts("merge_both") == sets("merge_both")[1:]            # i goes before j is asked
    assert len(pts("box_face")) == 1 and len(pts("box_apart")) == 2
    b = pl.oracle("edges/box_face")[2]["nodes"]
    assert b[0]["box"][0][1][0] == 1.0 == b[1]["box"][0][0][0]     # i's largest x is j's smallest
    b = pl.oracle("edges/box_apart")[2]["nodes"]
    assert b[1]["box"][0][0][0] == np.nextafter(b[0]["box"][0][1][0], 2.0)
    wp, wm, _ = pl.oracle("edges/repre")
    assert [len(x) for x in wm] == [70, 3]
    cov = [c for _, c in wm[0]]
    order = sorted(range(70), key=lambda i: cov[i], reverse=True)[:5]              # Python's stable sort, as :126-128
    assert order == pl.REPRE_TOP and cov[3] == cov[66] == cov[68] > cov[10] == cov[65] == cov[69] > max(cov[11:64])


@pytest.mark.parametrize("name", pl.DYADIC)
def test_oracle_dbscan_equals_scikit_learn(name):
    from scipy.spatial import cKDTree
    from sklearn.cluster import DBSCAN
    c, (_, _, det) = pl.built(name), pl.oracle(name)
    nodes = [n for n in c.onodes if len(n[0]) >= 2]
    for (masks, vf, order), r in zip(nodes, det["nodes"]):
        p = c.scene[order]
        pairs = cKDTree(p).query_pairs(2 * pl.EPS, output_type="ndarray")
        d = np.sqrt(((p[pairs[:, 0]] - p[pairs[:, 1]]) ** 2).sum(1))
        assert len(d) == 0 or np.abs(d - pl.EPS).min() >= MARGIN
        sk = DBSCAN(eps=pl.EPS, min_samples=pl.MIN_POINTS, algorithm="kd_tree").fit(p)
        lab = r["lab"] - 1
        np.testing.assert_array_equal(sk.labels_ == -1, lab == -1, err_msg="noise set")
        core = sk.core_sample_indices_
        pairs_of = sorted(set(zip(sk.labels_[core].tolist(), lab[core].tolist())))
        assert len(pairs_of) == len({a for a, _ in pairs_of}) == len({b for _, b in pairs_of})   # the same partition
