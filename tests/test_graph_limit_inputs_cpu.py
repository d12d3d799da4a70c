"""The inputs of test_gpu_graph_limits.py, checked without a GPU (graph_limit_inputs.py): the constants the
helper restates are the ones in maskclustering_amd/csrc, every case sits on the branch it is meant to pin,
every knife edge of S3 is hit exactly, the numpy restatement of S2/S3 equals the reference's own outputs on
the golden cases, and the dense and sparse CPU oracles (two separate restatements) agree with each other and
with the numpy one on the cases themselves."""
import os
import re

import numpy as np
import pytest

import graph_limit_inputs as gl
from conftest import CASES, load_case
from golden_compare import case_inputs
from maskclustering_amd.synthetic import SceneMasks

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "maskclustering_amd", "csrc")


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_restated_constants_are_the_sources():
    s3, plan, s4, host = _src("mc_s3_kernels.inl"), _src("mc_graph_plan.hpp"), _src("mc_s4_kernels.inl"), \
        _src("mc_graph_host.inl")
    for w, cfg in ((1, gl.S3_WAVE), (4, gl.S3_BIG)):
        m = re.search(r"S3Cfg<%d> \{ static constexpr int FWMAX = (\d+), CNT = (\d+), HS = (\d+), NT = 256; \}" % w, s3)
        assert m and tuple(map(int, m.groups())) == (cfg["FWMAX"], cfg["CNT"], cfg["HS"])
    assert re.search(r"#define MC_S3_BIGW %d\b" % gl.S3_BIG["W"], s3) and re.search(r"#define MC_S3_SMALL %d\b" % gl.S3_SMALL_PTS, s3)
    assert "return F <= 64 * lim.frame_words64 && max_per_frame < lim.counters;" in plan
    assert "constexpr size_t kHistReplicaBytes = 40 * 1024;" in plan and gl.HIST_REPLICA_BYTES == 40 * 1024
    assert "inline int hist_stride(int F) { return (F + 1) | 1; }" in plan
    assert "constexpr int kHistTile = 64, kHistKW = 8;" in s4 and gl.HIST_TILES_LDS == 2 * 64 * 8 * 8
    assert "constexpr size_t kS4ThrStaticLds = 256 * sizeof(unsigned long long) + 20 * sizeof(float);" in s4
    assert "kTestWords = %d" % gl.TEST_WORDS in _src("mc_s6_pairs.inl")
    assert "constexpr int kLocalBits = %d;" % gl.LOCAL_BITS in _src("mc_internal.hpp")
    assert "num_frames <= %d" % gl.MAX_FRAMES in host and "frame_masks[c] < %d" % (gl.MAX_PER_FRAME + 1) in host
    assert "sc.M <= %d" % gl.MAX_MASKS in host


def test_histogram_replicas_and_lds_requests():
    """hist_replicas falls from 32 to 1 and then stops fitting; the two S4 kernels' LDS at the most frames is
    above 64 KiB and below the 160 KiB a workgroup of an MI355X may ask for, so the host's check passes it."""
    assert [gl.hist_replicas(F) for F in (318, 319, 5118, 5119, 10238, 10239, 16384)] == [32, 16, 2, 1, 1, 1, 1]
    assert gl.hist_replica_fits(10238) and not gl.hist_replica_fits(10239)
    assert gl.hist_lds_bytes(16384) == 8192 + 4 * 16385 == 73732
    assert gl.thresholds_lds_bytes(16384) == 8 * 16385 + 2128 == 133208
    assert 64 * 1024 < gl.hist_lds_bytes(16384) < gl.thresholds_lds_bytes(16384) <= 160 * 1024


@pytest.mark.parametrize("name", list(gl.SCENES))
def test_case_sits_on_its_branch(name):
    gl.check_branch(name)


def test_case_f_and_g_inputs():
    for F, seed in ((2049, 0), (4100, 1), (16384, 2)):
        vf, cm, thr, ct = gl.case_f(F, seed)
        assert vf.shape == (300, F) and vf[:, F - 1].sum() >= 4 and vf[2].all() and cm.shape[0] == 300
        assert (F + 63) // 64 > 32 and ((F + 63) // 64) % gl.TEST_WORDS == (1, 1, 0)[seed]   # whole and partial chunks
    rows = gl.case_g()
    assert all(v.shape[1] == gl.MAX_FRAMES for v in rows.values())
    assert rows["all_ones"].all() and rows["one_bit"].sum(1).tolist() == [1, 1, 1]
    assert rows["last_bit"][:, -1].all() and rows["last_bit"].sum() == 3


@pytest.mark.parametrize("pad", [0, 2049 - 8])
def test_knife_edges_are_exact(pad):
    s, edges = gl.knife_scene(pad)
    assert gl.well_formed(s) and gl.s3_wave_ok(s.num_frames, gl.max_per_frame(s)) == (pad == 0)
    lists = gl.point_lists(s)
    assert not lists[0].any()                                     # no boundary point: T is the mask size
    # the two sides of each comparison, as float64: 1 - c0/T carries the rounding of a number near 1 (2^-54),
    # which is one step of the doubles above 0.3 and two steps of those below 0.2
    assert 1 - 7 / 10 == np.nextafter(0.3, 1) and 1 - 4 / 5 == 0.2 - 2.0 ** -54 == np.nextafter(np.nextafter(0.2, 0), 0)
    assert 4 / 5 == 0.8 and 2 / 4 == 0.5 and 1 - 1201 / 1700 < 0.3 and 1 - 510 / 1010 < 0.5
    for cfg_name, (mvt, ust, cont) in gl.KNIFE_CFGS.items():
        detail = {}
        r = gl.s3_restatement(s, mvt, ust, cont, detail=detail)
        for name, (label, f, c, T, nz, bc, want) in edges.items():
            if c != cfg_name:
                continue
            g = gl.global_index(s, 0, label)
            if f is None:                                         # under-segmentation: split / visible on 0.5
                assert (g in r["undersegment"]) == want, name
                continue
            assert detail[(g, f)][:3] == (T, nz, bc), name
            assert gl.decide(T, nz, bc, mvt, cont) == want, name
            assert r["vf"][g, f] == (want == 2), name
            kernel = gl.route(s, g, lists)["kernel"]
            assert kernel == ("wave" if pad == 0 and T <= gl.S3_SMALL_PTS else "workgroup"), name
        if cfg_name == "B":                                       # the tie goes to label 2, the second slot
            g = gl.global_index(s, 0, edges["tie"][0])
            assert detail[(g, 3)][3] == 2 and s.mask_label[gl.global_index(s, 3, 2) - 1] == 7
            assert gl.global_index(s, 3, 2) in r["c_col"][r["c_row"] == g]


def _same_s3(r, want, rows=None):
    vf_want = np.unpackbits(np.asarray(want["vf_bits"]), axis=1)[:, :r["vf"].shape[1]].astype(bool)
    rows = np.arange(len(vf_want)) if rows is None else np.asarray(rows)
    np.testing.assert_array_equal(r["boundary"], want["boundary"], err_msg="boundary")
    np.testing.assert_array_equal(r["vf"], vf_want[rows], err_msg="visible frames")
    sel = np.isin(want["c_row"], rows)
    np.testing.assert_array_equal(r["c_row"], np.asarray(want["c_row"])[sel], err_msg="contained rows")
    np.testing.assert_array_equal(r["c_col"], np.asarray(want["c_col"])[sel], err_msg="contained targets")
    np.testing.assert_array_equal(r["undersegment"], np.intersect1d(want["undersegment"], rows), err_msg="undersegment")


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_reference_on_golden_cases(name):
    z = load_case(name)
    inp = case_inputs(z)
    s = SceneMasks(inp["num_points"], inp["num_frames"], inp["mask_col"], inp["mask_label"], inp["mask_off"],
                   inp["mask_pts"])
    r = gl.s3_restatement(s, inp["mask_visible_threshold"], inp["undersegment_filter_threshold"],
                          inp["contained_threshold"])
    _same_s3(r, z)
    np.testing.assert_array_equal(s.mask_col[r["kept"]], z["gl_col"])
    for k, v in gl.dense_keys(r["pim"], r["pfm"]).items():
        np.testing.assert_array_equal(v, z[k], err_msg=k)


def _oracles(s, cfg, dense):
    from oracle import oracle
    args = (s.num_points, s.num_frames, s.mask_col, s.mask_label, s.mask_off, s.mask_pts)
    sparse = oracle.run_sparse(*args, **cfg)
    if dense:
        full = oracle.run(*args, **cfg)
        for k in full:
            if not k.startswith("pim_") and k != "pfm_bits":
                np.testing.assert_array_equal(np.asarray(sparse[k]), np.asarray(full[k]), err_msg=k)
        return sparse, full
    return sparse, None


@pytest.mark.parametrize("name", ["a2049", "b", "c", "d1023", "d2047"])
def test_oracles_and_restatement_agree_on_the_cases(name):
    """the dense oracle where it is affordable (M of a few thousand, P F of some ten million), against the sparse
    one on every key they share; the numpy restatement of the wide masks' rows against the sparse oracle, and
    its dense matrices against the dense oracle's"""
    s, cfg, wide = gl.built(name)
    sparse, full = _oracles(s, cfg, dense=name in ("a2049", "b", "c"))
    rows = sorted(wide) if wide else list(range(0, s.num_masks, 97))
    mats = gl.dense_matrices(s)
    r = gl.s3_restatement(s, cfg["mask_visible_threshold"], cfg["undersegment_filter_threshold"],
                          cfg["contained_threshold"], rows=rows, dense=mats)
    _same_s3(r, sparse, rows)
    if full is not None:
        for k, v in gl.dense_keys(mats[2], mats[3]).items():
            np.testing.assert_array_equal(v, full[k], err_msg=k)


@pytest.mark.parametrize("name", ["e5200", "e16384"])
def test_case_e_populates_the_last_bins(name):
    s, cfg, wide = gl.built(name)
    sparse, _ = _oracles(s, cfg, dense=False)
    h, F = sparse["observer_hist"], s.num_frames
    assert int(h[F]) == 9 and int(h[F - 1]) == 27 and len(sparse["undersegment"]) == 0
    vf = np.unpackbits(sparse["vf_bits"][list(wide)], axis=1)[:, :F]
    assert sorted(vf.sum(1).tolist()) == [F - 1] * 3 + [F] * 3


@pytest.mark.parametrize("pad", [0, 2049 - 8])
def test_oracles_agree_on_the_knife_scene(pad):
    s, _ = gl.knife_scene(pad)
    for mvt, ust, cont in gl.KNIFE_CFGS.values():
        cfg = dict(mask_visible_threshold=mvt, undersegment_filter_threshold=ust, view_consensus_threshold=0.9,
                   contained_threshold=cont)
        sparse, _ = _oracles(s, cfg, dense=True)
        _same_s3(gl.s3_restatement(s, mvt, ust, cont), sparse)
