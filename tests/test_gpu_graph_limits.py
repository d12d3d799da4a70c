"""The graph path at the frame and masks-per-frame limits it accepts (16384 frames, 2047 masks in a frame),
through the C-ABI against the CPU oracles and a numpy restatement of S2/S3 (graph_limit_inputs.py, whose
inputs and branch predicates test_graph_limit_inputs_cpu.py checks without a GPU).  Bit-exact: integer and
index work, float64 ratio tests and a float32 percentile with every operation rounded as numpy rounds it.

Every case asserts, from its inputs, the branch it is meant to take (graph_limit_inputs.check_branch) before
it compares anything, so a retuned constant fails the test instead of moving it off its branch.

  case    F      M      most masks  branch pinned                                           oracle   device
                        in a frame                                                          (CPU s)  (s)
  a2048   2048   3384   4           last frame count of the wave kernel k_s3_masks<1>       0.07     0.05
  a2049   2049   3386   4           first all-workgroup frame count, FW = 33                0.06     0.03
  b       2112   3479   5           workgroup kernel, hash path, 2 to 5 windows of 256      0.07     0.04
  c       2112   3479   5           workgroup kernel, s3_dense<4>, 8 and 9 windows          0.10     0.19
  d1023   24     6243   1023        last counter count of the wave kernel; s3_dense<1>      0.03     0.07
                                    windows of one crowded frame
  d1024   24     6249   1024        first all-workgroup count; s3_dense<4> windows of 3     0.03     0.07
  d2047   24     12387  2047        the most masks of a frame; windows of 2 and 1           0.09     0.25
  e5200   5200   5547   3           R = 1 histogram replica; bins F and F - 1 populated     0.04     0.11
  e16384  16384  16731  3           no replica fits kHistReplicaBytes; 72 KiB and 130 KiB   0.29     0.17
                                    of LDS; FW = 256; s3_dense<4> over 64 windows
  f       2049, 4100, 16384 (300 nodes)  k6_pairs popcounts with FW = 33, 65, 256           < 0.01   0.03
  g       16384 (3 to 61 rows)           mc_observer_thresholds, bins 1, 3, 16384           < 0.01   0.01
  knife   8 and 2049 (29 masks)          S3 decisions on a rule, wave and workgroup kernel  0.01     0.5 (6 runs)

The oracle column is oracle.run_sparse on the host's 16 threads (1.4 s for e16384 and 0.7 s for c on 8), the
device column mc_scene_set_masks + mc_graph_build + mc_cluster_run and the read-back of every compared array,
both as measured on an MI355X machine; the numpy restatement of a case's wide masks adds up to 1 s (c).

Case c is also the only scene of the suite in which thousands of level-0 nodes overflow k6_pairs' LDS hash
at once (every mask is contained in a wide one, so every node has every later node as a partner) and their
workgroups pass the 64 dense-counter slots from one to the next: its level-0 edge count was 31 short of the
oracle's 141392 until the counters' clears were fenced before the slot's release (mc_s6_pairs.inl)."""
import time

import numpy as np
import pytest

import graph_limit_inputs as gl
from cluster_check import oracle_cluster_check
from golden_compare import assert_matches
from test_gpu_large import KEYS

pytestmark = pytest.mark.gpu

DENSE_MAX = 5 * 10 ** 7   # P F up to which the dense point-in-mask / point-frame matrices are compared


@pytest.fixture(scope="module")
def run():
    from maskclustering_amd.pipeline import GraphRun
    return GraphRun(0)


_want, _got = {}, {}


def _reference(name):
    """oracle.run_sparse of a case, computed once and left unchanged"""
    if name not in _want:
        from oracle import oracle
        s, cfg, _ = gl.built(name)
        t = time.perf_counter()
        _want[name] = oracle.run_sparse(s.num_points, s.num_frames, s.mask_col, s.mask_label, s.mask_off, s.mask_pts,
                                        **cfg)
        print(f"{name}: oracle {time.perf_counter() - t:.2f} s")
    return _want[name]


def _device(run, name):
    """the device's canonical result of a case, computed once"""
    if name not in _got:
        s, cfg, _ = gl.built(name)
        t = time.perf_counter()
        run.set_scene(s)
        run.step(**cfg)
        _got[name] = run.canonical(dense=s.num_points * s.num_frames <= DENSE_MAX)
        print(f"{name}: device {time.perf_counter() - t:.2f} s")
    return _got[name]


def _compare(got, want):
    for k in KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "observer_hist":  # the device histogram skips O = 0 (not a percentile input)
            g, w = g[1:], w[1:]
        np.testing.assert_array_equal(g, w, err_msg=k)
    for t in range(int(want["num_iters"])):
        np.testing.assert_array_equal(got[f"part_{t}"], want[f"part_{t}"], err_msg=f"partition {t}")


@pytest.mark.parametrize("name", list(gl.SCENES))
def test_whole_path_vs_sparse_oracle(run, name):
    """S2 to S7 against oracle.run_sparse, every key of test_gpu_large.py and every iteration's partition;
    the dense point-in-mask and point-frame matrices (FW > 32 words) against the numpy restatement's"""
    gl.check_branch(name)
    s, cfg, wide = gl.built(name)
    want, got = _reference(name), _device(run, name)
    _compare(got, want)
    if s.num_points * s.num_frames <= DENSE_MAX:
        _, _, pim, pfm = gl.dense_matrices(s)
        for k, v in gl.dense_keys(pim, pfm).items():
            np.testing.assert_array_equal(got[k], v, err_msg=k)
    if name.startswith("e"):   # the observer counts F and F - 1 are populated bins
        F = s.num_frames
        assert got["observer_hist"][F] == 9 and got["observer_hist"][F - 1] == 27


@pytest.mark.parametrize("name", ["b", "c", "d1023", "d1024", "d2047"])
def test_s3_wide_masks_vs_restatement(run, name):
    """the wide masks' visible frames, contained rows and under-segmentation, and the boundary points,
    against the numpy restatement of the reference's text (a witness that shares nothing with the oracles)"""
    gl.check_branch(name)
    s, cfg, wide = gl.built(name)
    got = _device(run, name)
    rows = sorted(wide)
    r = gl.s3_restatement(s, cfg["mask_visible_threshold"], cfg["undersegment_filter_threshold"],
                          cfg["contained_threshold"], rows=rows)
    np.testing.assert_array_equal(got["boundary"], r["boundary"], err_msg="boundary")
    vf = np.unpackbits(got["vf_bits"][rows], axis=1)[:, :s.num_frames].astype(bool)
    np.testing.assert_array_equal(vf, r["vf"], err_msg="visible frames")
    sel = np.isin(got["c_row"], rows)
    np.testing.assert_array_equal(got["c_row"][sel], r["c_row"], err_msg="contained rows")
    np.testing.assert_array_equal(got["c_col"][sel], r["c_col"], err_msg="contained targets")
    np.testing.assert_array_equal(np.intersect1d(got["undersegment"], rows), r["undersegment"], err_msg="undersegment")


@pytest.mark.parametrize("pad", [0, 2049 - 8])
def test_s3_knife_edges(run, pad):
    """masks that sit exactly on a rule of S3 (graph_limit_inputs.knife_scene), in the wave kernel (8 frames)
    and, padded to 2049 frames, in the workgroup kernel: the restatement's decisions, and the dense oracle's
    whole result"""
    from oracle import oracle
    s, edges = gl.knife_scene(pad)
    assert gl.s3_wave_ok(s.num_frames, gl.max_per_frame(s)) == (pad == 0)
    for cfg_name, (mvt, ust, cont) in gl.KNIFE_CFGS.items():
        cfg = dict(mask_visible_threshold=mvt, undersegment_filter_threshold=ust, view_consensus_threshold=0.9,
                   contained_threshold=cont)
        run.set_scene(s)
        run.step(**cfg)
        got = run.canonical()
        r = gl.s3_restatement(s, mvt, ust, cont)
        vf = np.unpackbits(got["vf_bits"], axis=1)[:, :s.num_frames].astype(bool)
        for name, (label, f, c, T, nz, bc, want) in edges.items():
            if c != cfg_name:
                continue
            g = gl.global_index(s, 0, label)
            if f is None:
                assert (g in got["undersegment"]) == want, name
            else:
                assert vf[g, f] == (want == 2), name
        np.testing.assert_array_equal(vf, r["vf"], err_msg=cfg_name)
        np.testing.assert_array_equal(got["c_col"], r["c_col"], err_msg=cfg_name)
        np.testing.assert_array_equal(got["undersegment"], r["undersegment"], err_msg=cfg_name)
        assert_matches(got, oracle.run(s.num_points, s.num_frames, s.mask_col, s.mask_label, s.mask_off, s.mask_pts,
                                       **cfg))


def test_limits_are_refused_one_past(run):
    """2048 masks in a frame and 16385 frames are MC_ERR_UNSUPPORTED, not a wrong result"""
    from maskclustering_amd._native import McError, MC_ERR_UNSUPPORTED
    from maskclustering_amd.synthetic import SceneMasks
    crowd = SceneMasks.from_frame_lists(2048, [[(j + 1, [j]) for j in range(2048)]])
    frames = SceneMasks.from_frame_lists(4, [[(1, [0, 1])]] + [[] for _ in range(gl.MAX_FRAMES)])
    for s in (crowd, frames):
        with pytest.raises(McError) as e:
            run.set_scene(s)
        assert e.value.code == MC_ERR_UNSUPPORTED


@pytest.mark.parametrize("F,seed", [(2049, 0), (4100, 1), (16384, 2)])
def test_cluster_random_nodes_wide_rows(run, F, seed):
    """mc_nodes_set + mc_cluster_run with 33, 65 and 256 words per row against the dense oracle"""
    vf, cm, thr, ct = gl.case_f(F, seed)
    oracle_cluster_check(run, vf, cm, thr, ct)


def test_observer_thresholds_at_most_frames(run):
    """mc_observer_thresholds at F = 16384 (130 KiB of LDS in k_s4_thresholds, 72 KiB in k_s4_hist): rows of
    all ones (the last bin), of one bit, of bit 16383 alone, and a mixture"""
    from maskclustering_amd.pipeline import bool_to_bits
    from oracle import oracle
    for name, vf in gl.case_g().items():
        F = vf.shape[1]
        want, want_int = oracle.thresholds_from_hist(oracle.observer_hist(vf.astype(np.uint8)))
        thr, isint = run.ctx.observer_thresholds(bool_to_bits(vf), F)
        np.testing.assert_array_equal(thr.view(np.uint32), want.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(isint, want_int, err_msg=name)
