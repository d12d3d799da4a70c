"""Post-processing past 64 frames and at its window, node-size and slot limits (pp_limit_inputs.py, whose cases
test_pp_limit_inputs_cpu.py checks without a GPU), through mc_pp_run and mc_pp_run_device against the CPU
restatement (oracle/pp_oracle.py).  Bit-exact, without a tolerance anywhere: every compared value is an integer, a
coordinate copied from the input, or one IEEE division of two integers.

Per case and entry: the info counts, every array of mc_pp_get_results for every DBSCAN object and every mask of
every node (kept or not), and the export (point lists, mask lists, float64 coverages, obj_repre, the [P, K]
prediction matrix, host and device copies).

Each case catches a one-token change of the kernels made for it; each was built into a library of its own and
this file run against it once on an MI355X, where exactly the tests named failed (as comparisons, not faults):

  change (k_pp_filter, pp_wave_argmax: mc_pp_filter.inl; k_pp_prep,
  k_pp_cl_gather: mc_pp_layout.inl; k_pp_dbscan and its steps:
  mc_pp_dbscan.inl; k_pp_decide: mc_pp_merge.inl)                          tests that fail
  k_pp_filter: hit word  fp >> 6  ->  0                                    f65, f128, f129, f200, shifted, drop-in f129
  k_pp_prep: rank loop  w < (col >> 6)  ->  w < 0                          the same and the clustered entry
  k_pp_filter: cvid loop  w < FW  ->  w < 1                                the same
  k_pp_filter: cnode loop  w < W  ->  w < 1                                the same
  k_pp_cl_gather: w < FW  ->  w < 1                                        the clustered entry alone
  k_pp_dbscan (pp_grid): cell of  P - mn[c]  ->  P - 0.0                   shifted (and the other cases off the origin)
  k_pp_filter step 3: obj_box[ob + c0 + c]  ->  [ob + 0 + c]               obj257, obj1025, obj2049 alone
  k_pp_filter step 2: c0 += kPPObjChunk  ->  c0 += no  (one window)        obj1025, obj2049 alone
  pp_wave_argmax: oi < ix  ->  oi > ix                                     obj1025, obj2049 (and every other tie)
  k_pp_dbscan, global branch: uf_unite(pa, i, j)  ->  (pa, i, i)           test_n8193_on_each_dbscan_path[8193] alone
  k_pp_dbscan step 5:  < pr.eps2  ->  <=                                   edges eps_at alone
  k_pp_filter:  > pr.thr  ->  >=                                           edges ratio_at alone
  k_pp_decide:  / len[i] > pr.ratio  ->  >=                                edges merge_4_of_5 (and slots40)
  k_pp_decide:  bi[d] > bj[3 + d]  ->  >=   /   bj[d] > bi[3 + d]  ->  >=  edges merge_both   /   box_face, merge_*

Three changes the cases are also for were not run on a device, because the changed kernel would index out of
bounds or read slots nobody wrote: v > largest -> v >= largest (a window that misses the mask then gives object
c0 + INT_MAX; (a) of obj1025 is the case for it), o - c0 -> o in step 3 (an LDS index past the window; obj257), and
pp_merge without its regrow (k_pp_pairs reads the unwritten slots 17..; slots17, slots40, whose reach is asserted
from the oracle's lists before the merge).
"""
import functools
import time

import numpy as np
import pytest

import pp_limit_inputs as pl
from test_gpu_pp import _check, _node
from test_gpu_pp_device import RESULT_KEYS, _check_export, _info, _params, _run_device, _run_host

pytestmark = pytest.mark.gpu

K = pl.constants()


@functools.lru_cache(maxsize=None)
def _ctx():
    from maskclustering_amd import _native
    return _native.Context(0)


@functools.lru_cache(maxsize=None)
def _args(name):
    return pl.pack_arrays(*pl.built(name).inputs)


def _equals_oracle(ctx, name):
    """the context's result against the oracle's: info, every result array, the export"""
    c, want = pl.built(name), pl.expected_results(name)
    wp, wm, _ = pl.oracle(name)
    assert _info(ctx) == want["info"]
    res = ctx.pp_results()
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(res[k], want[k], err_msg=f"{name}: {k}")
    _check_export(ctx, len(c.scene), wp, wm)
    return res


def _both_entries(name):
    ctx, c = _ctx(), pl.built(name)
    pl.oracle(name)                                                   # computed once, outside the device's time
    t = time.perf_counter()
    _run_host(ctx, _params(c.thr), _args(name))
    res = _equals_oracle(ctx, name)
    _run_device(ctx, _params(c.thr), _args(name))
    _equals_oracle(ctx, name)
    print(f"{name}: both entries, compared, {time.perf_counter() - t:.2f} s")
    return res


@pytest.mark.parametrize("name", ["f65", "f128", "f129", "f200"])
def test_frame_words(name):
    _both_entries(name)


def test_shifted_scene():
    a = _both_entries("f65")
    b = _both_entries("shifted")
    for k in RESULT_KEYS:
        if k != "object_bbox":
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    np.testing.assert_array_equal(b["object_bbox"] - np.tile(np.asarray(pl.SHIFT), 2), a["object_bbox"])


@pytest.mark.parametrize("name", ["obj257", "obj1025", "obj2049"])
def test_object_windows(name):
    _both_entries(name)


@pytest.mark.parametrize("name", ["n8192", "n8193"])
def test_node_sizes(name):
    _both_entries(name)


@pytest.mark.parametrize("big_min", [None, K["kPPLdsUF"] + 1, 500])
def test_n8193_on_each_dbscan_path(big_min, monkeypatch):
    """the default (the 8193-point node split over the chip), MC_PP_BIG_MIN = kPPLdsUF + 1 (the same node in
    k_pp_dbscan on its global-memory union-find, the only way to that branch) and 500 (the 511, 512 and 513-point
    nodes split too): each equals the oracle, so all three are identical"""
    if big_min is None:
        monkeypatch.delenv("MC_PP_BIG_MIN", raising=False)
    else:
        monkeypatch.setenv("MC_PP_BIG_MIN", str(big_min))
    sizes = pl.built("n8193").meta["sizes"]
    assert pl.big_items(sizes, K["kPPLdsUF"] if big_min is None else big_min)[0] == {None: 1, 500: 4}.get(big_min, 0)
    _both_entries("n8193")


@pytest.mark.parametrize("name", ["slots17", "slots40"])
def test_slots_regrow(name):
    assert pl.most_objects_on_a_point(name) > K["kPPSlots"]
    _both_entries(name)


@pytest.mark.parametrize("name", list(pl.EDGE_CASES))
def test_rule_edges(name):
    _both_entries("edges/" + name)
    if name == "repre":
        r = _ctx().pp_export()
        assert r["obj_repre"][0].tolist() == pl.REPRE_TOP and r["obj_repre"][1].tolist() == [2, 0, 1, -1, -1]


@pytest.mark.parametrize("name", ["border_y_first", "border_x_first", "noise_last", "noise_none", "no_core"])
def test_rule_edges_on_split_route(name, monkeypatch):
    """MC_PP_BIG_MIN = 1 sends these nodes of 3 to 9 points through k_pp_big_grid, k_pp_big_walk and k_pp_big_label:
    the border rule, the noise class with and without members, and a node without a core point through the shared
    steps' second caller and the bucket-list walk (the n8193 nodes hold no border point and only one noise point)"""
    monkeypatch.setenv("MC_PP_BIG_MIN", "1")
    sizes = [len(n[2]) for n in pl.built("edges/" + name).onodes]
    assert pl.big_items(sizes, 1)[0] == len(sizes)
    _both_entries("edges/" + name)


def test_extent_limit():
    from maskclustering_amd import _native
    ctx = _ctx()
    _both_entries("wide")                                             # 2^21 - 2 cells: accepted
    refused = pl.pack_arrays(*pl.WIDE_REFUSED().inputs)
    for run, after in ((_run_host, "edges/eps_below"), (_run_device, "wide")):
        with pytest.raises(_native.McError) as e:
            run(ctx, _params(0.0), refused)                           # 2^21 - 1 cells
        assert e.value.code == _native.MC_ERR_UNSUPPORTED
        with pytest.raises(_native.McError) as e:
            ctx.pp_info()                                             # the refused call left no result
        assert e.value.code == _native.MC_ERR_STATE
        _both_entries(after)                                          # and the context runs the next case correctly


def _dropin(name):
    """a case as the drop-in's arguments: nodes with (frame id, mask id) lists, a dict of point sets"""
    c = pl.built(name)
    fids = [10 * f for f in range(c.pfm.shape[1])]
    key = lambda m: (fids[c.mask_col[m]], m + 1)  # noqa: E731
    mpc = {"%d_%d" % key(m): set(p.tolist()) for m, p in enumerate(c.mask_pts)}
    nodes = [_node([key(m) for m in masks], vf, order) for masks, vf, order in c.onodes]
    return nodes, mpc, fids, key


@pytest.mark.parametrize("name", ["f129"] + ["edges/" + n for n in pl.EDGE_CASES])
def test_dropin_entry(name):
    """post_process_objects of the drop-in (dict of sets, the Python packing of the bit rows and their tail)"""
    from maskclustering_amd.utils import post_process
    c = pl.built(name)
    nodes, mpc, fids, key = _dropin(name)
    got = post_process.post_process_objects(nodes, mpc, c.scene, c.pfm, fids, c.thr)
    wp, wm, _ = pl.oracle(name)
    _check(got, wp, [[(*key(m), cov) for m, cov in ml] for ml in wm])


# ---- the clustered entry past 64 frames ---------------------------------------------------------------
CL = dict(num_points=3000, num_frames=100, num_objects=24, win=0.6, seed=5)
CL_CFG = dict(mask_visible_threshold=0.3, undersegment_filter_threshold=0.3, view_consensus_threshold=0.9,
              contained_threshold=0.8)
CL_PRM = (0.1, 4, 0.6, 0.8)


def test_clustered_entry_two_frame_words():
    """mc_scene_set_masks, mc_graph_build, mc_cluster_run and mc_pp_run_clustered on a scene of 100 frames: against
    mc_pp_run on the node arrays rebuilt from the getters, and against the oracle on them"""
    from maskclustering_amd._native import PPParams
    from maskclustering_amd.pipeline import GraphRun, bits_to_bool
    from maskclustering_amd.synthetic import make_scene
    from oracle import pp_oracle
    s = make_scene(**CL)
    P, F = s.num_points, s.num_frames
    rng = np.random.default_rng(CL["seed"])
    scene = rng.integers(-45, 46, (P, 3)) * pl.U + np.stack([np.arange(P) // 100, np.zeros(P), np.zeros(P)], axis=1)
    run = GraphRun(0)
    run.set_scene(s)
    run.step(**CL_CFG)
    ctx = run.ctx
    ctx.pp_run_clustered(PPParams(*CL_PRM), scene)
    info, res = _info(ctx), ctx.pp_results()
    got = run.canonical(dense=False)
    mo, po = got["obj_mask_off"], got["obj_pt_off"]
    rows = got["_input_index"][got["obj_mask_idx"]]
    vf = np.unpackbits(got["obj_vf_bits"], axis=1)[:, :F].astype(bool)
    onodes = [(rows[mo[k]:mo[k + 1]].tolist(), vf[k], np.asarray(got["obj_pt_idx"][po[k]:po[k + 1]], np.int64))
              for k in range(len(mo) - 1)]
    mask_pts = [np.asarray(s.mask_points(g), np.int64) for g in range(s.num_masks)]
    pfm = bits_to_bool(ctx.point_frame_bits(P, F), F)
    wp, wm = pp_oracle.post_process_objects(scene, pfm, mask_pts, s.mask_col, onodes, CL_PRM[2], eps=CL_PRM[0],
                                            min_points=CL_PRM[1], overlapping_ratio=CL_PRM[3])
    assert len(wp) == info[2] >= 5
    r = _check_export(ctx, P, wp, wm)
    nodes = [n for n in onodes if len(n[0]) >= 2]
    two_words = [k for k in r["obj_node"] if nodes[k][1][:64].any() and nodes[k][1][64:].any()]
    assert two_words                                                  # FW = 2 in a final object's node
    # W = 2 as well, and it matters: points of final objects whose ratio decision turns on hits past rank 63
    decisive, final_nodes = 0, set(r["obj_node"].tolist())
    for k, (masks, vfk, order) in enumerate(nodes):
        vcols = np.nonzero(vfk)[0]
        if k not in final_nodes or len(vcols) <= 64:
            continue
        hit = np.zeros((P, len(vcols)), bool)
        for m in masks:
            hit[mask_pts[m], np.searchsorted(vcols, s.mask_col[m])] = True
        h, seen = hit[order], pfm[order][:, vcols].sum(1) + 1e-6
        decisive += int(((h.sum(1) / seen > CL_PRM[2]) != (h[:, :64].sum(1) / seen > CL_PRM[2])).sum())
    most = max(int(nodes[k][1].sum()) for k in final_nodes)
    print(f"clustered entry: {len(wp)} final objects, {len(two_words)} over two words, at most {most} visible frames, "
          f"{decisive} decisive points")
    assert decisive > 0
    _run_host(ctx, PPParams(*CL_PRM), pl.pack_arrays(scene, pfm, mask_pts, s.mask_col, onodes))
    assert _info(ctx) == info
    for k in RESULT_KEYS:
        np.testing.assert_array_equal(ctx.pp_results()[k], res[k], err_msg=k)
    _check_export(ctx, P, wp, wm)
