"""The S1 CPU restatement (oracle/s1_oracle.c) against an independent witness (s1_witness.py: numpy,
longdouble, written from the reference's Python and the libraries' published algorithms, not from the oracle),
and the witness against scikit-learn's DBSCAN and scipy's cKDTree: three implementations by different hands.
Whole frames (statistics columns and every mask's point set) and stage by stage (voxel means, DBSCAN labels
and outlier keep flags point by point, through the oracle's orc_s1_voxel / orc_s1_dbscan / orc_s1_sor), at
the reference's parameters and at every parameter variant of the device tests
(test_gpu_s1_denoise_edges.py).  Every compared input is free of knife-edge decisions under the parameters
it is compared at (s1_witness.knife_edges; the one exception, of an older input, is KNOWN_EDGES below), so the
comparisons are exact; none skips or masks a slot."""
import os

import numpy as np
import pytest

import s1_denoise_inputs as D
import s1_witness as W
from conftest import GOLDEN

ORACLE_COLS = [0, 1, 2, 3, 4, 6, 7, 8]  # id npix nvox ndbscan nsor ncovered nneighbors kept (W.STAT_NAMES)
VARIANTS = list(D.VARIANTS)


def _inputs(name):
    if name == "denoise":
        return D.denoise_inputs()
    if name in ("s1_tiny", "s1_dense"):
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        return z["in_scene"], z["in_depth"], z["in_seg"], z["in_intrinsics"], z["in_poses"]
    if name == "knnsel":
        from s1_knnsel_inputs import knnsel_inputs
        return knnsel_inputs()
    from s1_list_inputs import dense_inputs
    return dense_inputs()["tiny"]


INPUTS = ["denoise", "s1_tiny", "s1_dense", "knnsel", "tiny"]
# Knife edges of inputs from before the witness, (input, stage).  The k-NN selection inputs' lattice walls are
# 64 and 72 pixels wide: 32 lattice steps of 3 * 2^-8 from a slot's minimum, (p - vmin) / voxel =
# (0.375 + 0.005) / 0.01 is the integer 38 but for its roundings.  The comparison is made all the same and
# holds: the witness, the oracle and the kernels evaluate this one float64 expression, on lattice points that
# are exact in any order of the back-projection.
KNOWN_EDGES = {("knnsel", "voxel")}


@pytest.fixture(scope="module")
def inputs():
    return {n: _inputs(n) for n in INPUTS}


@pytest.fixture(scope="module")
def witnessed(inputs):
    """(input, variant) -> the witness's frames, computed once"""
    cache = {}

    def get(name, variant):
        if (name, variant) not in cache:
            scene, depth, seg, K, T = inputs[name]
            cache[name, variant] = W.frames(scene, depth, seg, K, T, **D.VARIANTS[variant])
        return cache[name, variant]
    return get


@pytest.mark.parametrize("variant", VARIANTS)
def test_denoise_inputs_meet_their_conditions(inputs, witnessed, variant):
    rep, margins = D.check_inputs(inputs["denoise"], witnessed("denoise", variant), **D.VARIANTS[variant])
    print(variant, rep, margins)


def _oracle_frames(inp, prm):
    from oracle import oracle
    scene, depth, seg, K, T = inp
    oprm = oracle.BpParams.default(**W.abi_params(prm))
    return oracle.s1_frames(np.asarray(scene, np.float64).astype(np.float32), list(depth), list(seg), K, T, oprm)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", INPUTS)
def test_oracle_frames_match_witness(inputs, witnessed, name, variant):
    wit = witnessed(name, variant)
    slots = [s for fr in wit for s in fr.values()]
    assert [e for e in W.knife_edges(slots) if (name, e[1]) not in KNOWN_EDGES] == []
    ref = _oracle_frames(inputs[name], D.VARIANTS[variant])
    assert len(ref) == len(wit)
    for f, (ol, oo, op, ost) in enumerate(ref):
        want = np.array([W.stats_row(s) for s in wit[f].values()], np.int64).reshape(-1, len(W.STAT_NAMES))
        np.testing.assert_array_equal(ost[:, ORACLE_COLS], want, err_msg=f"{name} frame {f}: {W.STAT_NAMES}")
        kept = [s for s in wit[f].values() if s["kept"]]
        assert [s["id"] for s in kept] == ol.tolist(), f
        for k, s in enumerate(kept):
            np.testing.assert_array_equal(op[oo[k]:oo[k + 1]], s["points"], err_msg=f"{name} frame {f} id {s['id']}")


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", ["denoise", "s1_dense"])
def test_oracle_stages_match_witness_point_by_point(inputs, witnessed, name, variant):
    from oracle import oracle
    prm = dict(W.DEFAULTS, **D.VARIANTS[variant])
    n = 0
    for f, fr in enumerate(witnessed(name, variant)):
        for i, s in fr.items():
            if s["means"] is None:
                continue
            tag = f"{name} frame {f} id {i}"
            vox = oracle.s1_voxel(s["world"], prm["voxel"])
            assert vox.shape == s["means"].shape, tag
            # the means: the same voxels in the same order; a sequential float64 sum of c points against the
            # longdouble one differs by at most c roundings of the running sum
            c = max(1, s["npix"])
            np.testing.assert_allclose(vox, s["means"].astype(np.float64), rtol=0, atol=c * 2.0 ** -52 * np.abs(vox).max(),
                                       err_msg=tag)
            labels = oracle.s1_dbscan(vox, prm["eps"], prm["min_points"])
            np.testing.assert_array_equal(labels, s["labels"], err_msg=tag + " DBSCAN labels")
            keep = oracle.s1_sor(vox, s["filtered"], prm["k"], prm["std_ratio"])
            np.testing.assert_array_equal(keep, s["sor"]["keep"], err_msg=tag + " outlier keep flags")
            n += 1
    assert n >= 20


def test_dbscan_labels_match_sklearn(inputs, witnessed):
    """scikit-learn's DBSCAN on the witness's own predicate matrix (so no distance is recomputed): the same
    labels, border assignments and cluster numbers included, at min_points 3, 4 and 6"""
    cluster = pytest.importorskip("sklearn.cluster")
    n = contested = 0
    for name in ("denoise", "s1_dense"):
        for variant, mp in (("min_points_3", 3), ("default", 4), ("min_points_6", 6)):
            for fr in witnessed(name, variant):
                for s in fr.values():
                    if s["means"] is None:
                        continue
                    db = W.dbscan(s["means"], 0.04, mp)
                    np.testing.assert_array_equal(db["labels"], s["labels"])
                    sk = cluster.DBSCAN(metric="precomputed", eps=0.5, min_samples=mp).fit(1.0 - db["adj"])
                    np.testing.assert_array_equal(sk.labels_, db["labels"], err_msg=f"{name} {variant} id {s['id']}")
                    core = np.zeros(len(db["labels"]), bool)
                    core[sk.core_sample_indices_] = True
                    np.testing.assert_array_equal(core, db["core"])
                    for b in np.nonzero(~core)[0]:
                        contested += len(set(db["labels"][db["adj"][b] & core].tolist())) >= 2
                    n += 1
    assert n >= 60 and contested >= 4


def test_outlier_decisions_match_ckdtree(inputs, witnessed):
    """scipy's cKDTree k-NN distances (float64) under the same threshold rule: the witness's keep flags"""
    spatial = pytest.importorskip("scipy.spatial")
    n = 0
    for name in ("denoise", "s1_dense"):
        for variant in ("default", "k_8", "k_19", "std_ratio_0.5"):
            prm = dict(W.DEFAULTS, **D.VARIANTS[variant])
            for fr in witnessed(name, variant):
                for s in fr.values():
                    if s["means"] is None:
                        continue
                    p = s["means"][s["filtered"]].astype(np.float64)
                    kk = min(prm["k"], len(p))
                    d, _ = spatial.cKDTree(p).query(p, k=kk)
                    v = d.reshape(len(p), kk).sum(axis=1) / kk
                    keep, _ = W.sor_keep(v, prm["std_ratio"])
                    np.testing.assert_array_equal(keep, s["sor"]["keep"], err_msg=f"{name} {variant} id {s['id']}")
                    n += 1
    assert n >= 80


def test_ball_sets_match_ckdtree(inputs, witnessed):
    """scipy's query_ball_point over the cropped scene points: the witness's balls before the cut to ball_k"""
    spatial = pytest.importorskip("scipy.spatial")
    n = over = 0
    for name in ("denoise", "s1_dense"):
        scene32 = np.asarray(inputs[name][0], np.float64).astype(np.float32)
        for fr in witnessed(name, "default"):
            for s in fr.values():
                if s["q32"] is None:
                    continue
                cand, _ = W.crop(s["q32"], scene32)
                hit, _ = W.ball_hits(s["q32"], scene32, cand, 0.01)
                if len(cand) == 0:
                    assert s["ncovered"] == 0
                    continue
                balls = spatial.cKDTree(scene32[cand].astype(np.float64)).query_ball_point(
                    s["q32"].astype(np.float64), float(np.float32(0.01)))
                for q, ball in enumerate(balls):
                    assert sorted(ball) == np.nonzero(hit[q])[0].tolist(), (name, s["id"], q)
                over += int((hit.sum(axis=1) > 20).any())
                n += 1
    assert n >= 20 and over >= 1


def test_witness_imports_nothing_of_the_oracle():
    """the witness imports nothing of the oracle, the golden maker or the list inputs' restatement"""
    src = open(W.__file__).read()
    body = src.split('"""', 2)[2]
    for word in ("oracle", "make_s1_golden", "s1_list_inputs", "import ctypes"):
        assert word not in body, word
