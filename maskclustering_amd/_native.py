"""ctypes binding of libmcgraph.so (the C-ABI in include/mcgraph.h).

The library is built in-tree by ``__graft_entry__.build()`` (hipcc, gfx950).
There is no fallback: if the shared object is missing or fails to load, every
entry point raises, so a GPU run can never silently take another path.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCGRAPH_LIB") or os.path.join(HERE, "libmcgraph.so")  # override: profiling variants

MC_OK = 0
MC_ERR_INVALID = 1
MC_ERR_HIP = 2
MC_ERR_STATE = 3
MC_ERR_EMPTY_OBSERVERS = 4
MC_ERR_UNSUPPORTED = 5
MC_ERR_NO_NODES = 6

EXPORTED = [
    "mc_ctx_create", "mc_ctx_destroy", "mc_ctx_set_stream", "mc_ctx_get_stream", "mc_ctx_synchronize",
    "mc_ctx_last_error", "mc_ctx_set_timing", "mc_ctx_set_timing_filter", "mc_ctx_get_kernel_time", "mc_ctx_reset_kernel_times",
    "mc_debug_counters", "mc_ctx_set_memory_budget", "mc_scene_set_masks", "mc_graph_build", "mc_graph_get_info", "mc_graph_get_global_masks",
    "mc_graph_get_boundary", "mc_graph_get_point_in_mask", "mc_graph_get_point_frame_bits",
    "mc_graph_get_visible_frame_bits", "mc_graph_get_contained", "mc_graph_get_undersegment",
    "mc_graph_get_nodes0", "mc_graph_get_observer_hist", "mc_graph_get_thresholds", "mc_observer_thresholds",
    "mc_nodes_set",
    "mc_cluster_run", "mc_cluster_get_info", "mc_cluster_get_level_sizes", "mc_cluster_get_level_caps", "mc_cluster_get_partition",
    "mc_cluster_get_edge_counts", "mc_cluster_get_final_labels", "mc_cluster_get_objects",
    "mc_bp_params_default", "mc_scene_set_points", "mc_backproject", "mc_backproject_frames", "mc_backproject_frames_raw",
    "mc_backproject_get_info", "mc_backproject_get_batching",
    "mc_backproject_get_masks", "mc_backproject_get_candidates", "mc_backproject_get_voxels",
    "mc_scene_use_backprojection",
    "mc_backproject_copy_points_device",
    "mc_pp_run", "mc_pp_get_info", "mc_pp_get_results", "mc_pp_run_device", "mc_pp_run_clustered",
    "mc_pp_export_info", "mc_pp_export", "mc_pp_export_pred_masks", "mc_eval_match_counts", "mc_frames_decode",
    "mc_shard_set", "mc_shard_pending", "mc_shard_export", "mc_shard_import",
    "mc_cluster_set_edge_capture", "mc_cluster_get_edges", "mc_openvoc_query", "mc_bits_unpack", "mc_setorder_replay",
    "mc_setorder_begin", "mc_setorder_finish", "mc_setorder_free",
    "mc_comm_unique_id", "mc_ctx_comm_init", "mc_ctx_attach_comm",
    "mc_ev_begin", "mc_ev_add_scan", "mc_ev_add_scan_clustered", "mc_ev_add_matches", "mc_ev_scan_info", "mc_ev_get_scan",
    "mc_ev_ap", "mc_ev_get_curve", "mc_ev_state_info", "mc_ev_state_export", "mc_ev_state_merge",
    "mc_crop_params_default", "mc_crop_boxes", "mc_crop_render", "mc_crop_coeffs",
    "mc_proj_boxes", "mc_proj_top_views",
    "mc_cloud_params_default", "mc_cloud_fuse_frames", "mc_cloud_voxel_down", "mc_cloud_info", "mc_cloud_get",
    "mc_scene_use_cloud",
    "mc_paint_params_default", "mc_labels_paint",
]
MC_COMM_ID_BYTES = 128

MC_SHARD_S3 = 1
MC_SHARD_HIST = 2
MC_SHARD_FOREST = 3

MC_BP_NSTAT = 10
BP_STATS = ["frame", "id", "npix", "nvox", "ndbscan", "nsor", "ncand", "ncovered", "nneighbors", "kept"]


class McError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmcgraph error {code}: {msg}")
        self.code = code


class GraphParams(ctypes.Structure):
    _fields_ = [("mask_visible_threshold", ctypes.c_double),
                ("contained_threshold", ctypes.c_double),
                ("undersegment_filter_threshold", ctypes.c_double)]


class GraphInfo(ctypes.Structure):
    _fields_ = [("num_points", ctypes.c_int64), ("num_frames", ctypes.c_int32), ("num_masks", ctypes.c_int32),
                ("num_undersegment", ctypes.c_int32), ("num_nodes0", ctypes.c_int32),
                ("num_contained", ctypes.c_int64), ("num_boundary", ctypes.c_int64),
                ("num_thresholds", ctypes.c_int32), ("threshold_status", ctypes.c_int32)]


class ClusterInfo(ctypes.Structure):
    _fields_ = [("num_iterations", ctypes.c_int32), ("num_objects", ctypes.c_int32),
                ("num_nodes0", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("num_object_points", ctypes.c_int64), ("num_object_contained", ctypes.c_int64),
                ("num_object_masks", ctypes.c_int64)]


class BpParams(ctypes.Structure):
    """mc_bp_params: the S1 constants (utils/mask_backprojection.py:8-14,38; utils/geometry.py:10,16,22)."""
    _fields_ = [("depth_trunc", ctypes.c_double), ("voxel_size", ctypes.c_double),
                ("dbscan_eps", ctypes.c_double), ("component_min_fraction", ctypes.c_double),
                ("sor_std_ratio", ctypes.c_double), ("ball_radius", ctypes.c_double),
                ("coverage_threshold", ctypes.c_double), ("dbscan_min_points", ctypes.c_int32),
                ("sor_neighbors", ctypes.c_int32), ("ball_k", ctypes.c_int32), ("few_points", ctypes.c_int32)]


class BpInfo(ctypes.Structure):
    _fields_ = [("num_frames", ctypes.c_int32), ("num_candidates", ctypes.c_int32), ("num_masks", ctypes.c_int32),
                ("error_frame", ctypes.c_int32), ("num_mask_points", ctypes.c_int64)]


class PPParams(ctypes.Structure):
    """mc_pp_params: utils/post_process.py:104,109 (DBSCAN), :95 (point filter), :194 (overlap)."""
    _fields_ = [("dbscan_eps", ctypes.c_double), ("dbscan_min_points", ctypes.c_int32),
                ("point_filter_threshold", ctypes.c_double), ("overlapping_ratio", ctypes.c_double)]


class PPInfo(ctypes.Structure):
    _fields_ = [("num_objects", ctypes.c_int32), ("num_filtered", ctypes.c_int32), ("num_final", ctypes.c_int32),
                ("num_entries", ctypes.c_int64), ("num_node_masks", ctypes.c_int64)]


class CropParams(ctypes.Structure):
    """mc_crop_params: output side, levels and expansion (get_open-voc_features.py:18,66), the Normalize
    mean / std and the pad colour (:78)."""
    _fields_ = [("out_size", ctypes.c_int32), ("levels", ctypes.c_int32), ("expansion", ctypes.c_double),
                ("mean", ctypes.c_float * 3), ("std", ctypes.c_float * 3), ("pad_rgb", ctypes.c_uint8 * 3)]


MC_CROP_OK, MC_CROP_ABSENT, MC_CROP_EMPTY = 0, 1, 2


class CloudParams(ctypes.Structure):
    """mc_cloud_params: the voxel size (what tasmap2mct_format.py:240 calls depth_trunc=0.005), the depth
    limit (its DEPTH_LIMIT = 20) and the frames of a buffer (buffer_size)."""
    _fields_ = [("voxel_size", ctypes.c_double), ("depth_trunc", ctypes.c_double), ("buffer_frames", ctypes.c_int32)]


class PaintParams(ctypes.Structure):
    """mc_paint_params: the score threshold (mask_predict.py's --confidence-threshold) and the smallest
    area that is painted (:108)."""
    _fields_ = [("score_threshold", ctypes.c_float), ("min_pixels", ctypes.c_int32)]


MC_PAINT_OK, MC_PAINT_OVERFLOW = 0, 1
MC_PAINT_MAX_INSTANCES = 1024
MC_PAINT_MAX_IDS = 255
MC_PAINT_U8, MC_PAINT_F32 = 0, 1


_lib = None


def load():
    """Load libmcgraph.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same soname as
    # /opt/rocm's).  Whichever is loaded first serves both, and torch cannot initialise the GPU
    # on a runtime it was not built with, so torch's is loaded before this library when present.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, dbl = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    P = ctypes.POINTER
    sig = {
        "mc_ctx_create": (ctypes.c_int, [ctypes.c_int, P(vp)]),
        "mc_ctx_destroy": (None, [vp]),
        "mc_ctx_set_stream": (ctypes.c_int, [vp, vp]),
        "mc_ctx_get_stream": (vp, [vp]),
        "mc_ctx_synchronize": (ctypes.c_int, [vp]),
        "mc_ctx_last_error": (ctypes.c_char_p, [vp]),
        "mc_ctx_set_timing": (ctypes.c_int, [vp, ctypes.c_int]),
        "mc_ctx_set_timing_filter": (ctypes.c_int, [vp, ctypes.c_char_p]),
        "mc_ctx_get_kernel_time": (ctypes.c_int, [vp, ctypes.c_char_p, P(dbl), P(i64)]),
        "mc_ctx_reset_kernel_times": (ctypes.c_int, [vp]),
        "mc_debug_counters": (ctypes.c_int, [vp, vp, i32, ctypes.c_int]),
        "mc_ctx_set_memory_budget": (ctypes.c_int, [vp, i64]),
        "mc_scene_set_masks": (ctypes.c_int, [vp, i64, i32, i32, vp, vp, vp, vp, ctypes.c_int]),
        "mc_graph_build": (ctypes.c_int, [vp, P(GraphParams)]),
        "mc_graph_get_info": (ctypes.c_int, [vp, P(GraphInfo)]),
        "mc_graph_get_global_masks": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_boundary": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_point_in_mask": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_point_frame_bits": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_visible_frame_bits": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_contained": (ctypes.c_int, [vp, vp, vp]),
        "mc_graph_get_undersegment": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_nodes0": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_observer_hist": (ctypes.c_int, [vp, vp]),
        "mc_graph_get_thresholds": (ctypes.c_int, [vp, vp, vp, P(i32)]),
        "mc_observer_thresholds": (ctypes.c_int, [vp, i32, i32, vp, vp, vp, P(i32)]),
        "mc_nodes_set": (ctypes.c_int, [vp, i32, i32, i32, i64, vp, vp, vp, vp, vp]),
        "mc_cluster_run": (ctypes.c_int, [vp, vp, i32, dbl]),
        "mc_cluster_get_info": (ctypes.c_int, [vp, P(ClusterInfo)]),
        "mc_cluster_get_level_sizes": (ctypes.c_int, [vp, vp]),
        "mc_cluster_get_level_caps": (ctypes.c_int, [vp, vp]),
        "mc_cluster_get_partition": (ctypes.c_int, [vp, i32, vp]),
        "mc_cluster_get_edge_counts": (ctypes.c_int, [vp, vp]),
        "mc_cluster_get_final_labels": (ctypes.c_int, [vp, vp]),
        "mc_cluster_get_objects": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp]),
        "mc_bp_params_default": (None, [P(BpParams)]),
        "mc_scene_set_points": (ctypes.c_int, [vp, i64, vp, ctypes.c_int]),
        "mc_backproject": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, ctypes.c_int, P(BpParams)]),
        "mc_backproject_frames": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, P(BpParams)]),
        "mc_backproject_frames_raw": (ctypes.c_int, [vp, i32, i32, i32, vp, ctypes.c_double, vp, vp, vp, P(BpParams)]),
        "mc_backproject_get_info": (ctypes.c_int, [vp, P(BpInfo)]),
        "mc_backproject_get_batching": (ctypes.c_int, [vp, vp]),
        "mc_backproject_get_masks": (ctypes.c_int, [vp, vp, vp, vp, vp]),
        "mc_backproject_copy_points_device": (ctypes.c_int, [vp, vp]),
        "mc_backproject_get_candidates": (ctypes.c_int, [vp, vp]),
        "mc_backproject_get_voxels": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mc_scene_use_backprojection": (ctypes.c_int, [vp]),
        "mc_pp_run": (ctypes.c_int, [vp, P(PPParams), i64, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mc_pp_get_info": (ctypes.c_int, [vp, P(PPInfo)]),
        "mc_pp_get_results": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp]),
        "mc_pp_run_device": (ctypes.c_int, [vp, P(PPParams), i64, i32, vp, vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mc_pp_run_clustered": (ctypes.c_int, [vp, P(PPParams), vp, ctypes.c_int]),
        "mc_pp_export_info": (ctypes.c_int, [vp, P(i32), P(i64), P(i64)]),
        "mc_pp_export": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]),
        "mc_pp_export_pred_masks": (ctypes.c_int, [vp, vp, ctypes.c_int]),
        "mc_eval_match_counts": (ctypes.c_int, [vp, i64, i32, vp, vp, i32, vp, vp, vp, vp]),
        "mc_frames_decode": (ctypes.c_int, [vp, i32, i32, i32, vp, dbl, i32, i32, vp, ctypes.c_int, vp, vp]),
        "mc_shard_set": (ctypes.c_int, [vp, i32, i32]),
        "mc_cluster_set_edge_capture": (ctypes.c_int, [vp, i64]),
        "mc_openvoc_query": (ctypes.c_int, [vp, i32, vp, vp, i32, i32, vp, i32, vp, ctypes.c_float, vp]),
        "mc_bits_unpack": (ctypes.c_int, [vp, ctypes.c_int64, i32, i32, vp]),
        "mc_setorder_replay": (ctypes.c_int, [i32, vp, vp, vp, vp, vp, vp, i32, P(i32), vp, vp, vp, vp, vp, vp, vp]),
        "mc_setorder_begin": (ctypes.c_int, [i32, vp, vp, vp, i32, ctypes.c_int, P(vp)]),
        "mc_setorder_finish": (ctypes.c_int, [vp, i32, vp, vp, vp, vp, P(i32), vp, vp, vp, vp, vp, vp, vp]),
        "mc_setorder_free": (None, [vp]),
        "mc_cluster_get_edges": (ctypes.c_int, [vp, vp, P(i64)]),
        "mc_shard_pending": (ctypes.c_int, [vp, P(i32)]),
        "mc_shard_export": (ctypes.c_int, [vp, i32, vp, P(i64)]),
        "mc_shard_import": (ctypes.c_int, [vp, i32, vp, i64]),
        "mc_comm_unique_id": (ctypes.c_int, [vp]),
        "mc_ctx_comm_init": (ctypes.c_int, [vp, vp, i32, i32]),
        "mc_ctx_attach_comm": (ctypes.c_int, [vp, vp]),
        "mc_ev_begin": (ctypes.c_int, [vp, i32, vp, i32, vp, i64, ctypes.c_int]),
        "mc_ev_add_scan": (ctypes.c_int, [vp, i64, vp, i32, vp, i64, vp, vp, vp, ctypes.c_int]),
        "mc_ev_add_scan_clustered": (ctypes.c_int, [vp, vp, ctypes.c_int]),
        "mc_ev_add_matches": (ctypes.c_int, [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, i64, vp, vp, vp]),
        "mc_ev_scan_info": (ctypes.c_int, [vp, P(i32), P(i32), P(i64)]),
        "mc_ev_get_scan": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "mc_ev_ap": (ctypes.c_int, [vp, vp, vp]),
        "mc_ev_get_curve": (ctypes.c_int, [vp, i32, i32, P(i64), vp, vp, vp, vp]),
        "mc_ev_state_info": (ctypes.c_int, [vp, P(i64), P(i64), P(i64)]),
        "mc_ev_state_export": (ctypes.c_int, [vp, vp, i64, ctypes.c_int]),
        "mc_ev_state_merge": (ctypes.c_int, [vp, vp, i64, ctypes.c_int]),
        "mc_crop_params_default": (None, [P(CropParams)]),
        "mc_crop_boxes": (ctypes.c_int, [vp, i32, i32, i32, vp, ctypes.c_int, i32, vp, vp, P(CropParams), vp, vp,
                                         ctypes.c_int]),
        "mc_crop_render": (ctypes.c_int, [vp, i32, i32, i32, vp, ctypes.c_int, i32, vp, vp, vp, ctypes.c_int,
                                          P(CropParams), vp]),
        "mc_crop_coeffs": (ctypes.c_int, [vp, i32, i32, P(i32), vp, vp]),
        "mc_proj_boxes": (ctypes.c_int, [vp, i64, vp, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, ctypes.c_int, vp, vp,
                                         vp, ctypes.c_int]),
        "mc_proj_top_views": (ctypes.c_int, [vp, vp, i32, vp, vp, i32, i32, ctypes.c_int, i32, vp, vp, vp, vp, vp,
                                             ctypes.c_int]),
        "mc_cloud_params_default": (None, [P(CloudParams)]),
        "mc_cloud_fuse_frames": (ctypes.c_int, [vp, i32, i32, i32, vp, vp, vp, vp, ctypes.c_int, P(CloudParams)]),
        "mc_cloud_voxel_down": (ctypes.c_int, [vp, i64, vp, vp, dbl, ctypes.c_int]),
        "mc_cloud_info": (ctypes.c_int, [vp, vp]),
        "mc_cloud_get": (ctypes.c_int, [vp, vp, vp, ctypes.c_int]),
        "mc_scene_use_cloud": (ctypes.c_int, [vp]),
        "mc_paint_params_default": (None, [P(PaintParams)]),
        "mc_labels_paint": (ctypes.c_int, [vp, i32, i32, i32, vp, i32, vp, vp, ctypes.c_int, P(PaintParams), vp, vp, vp, vp,
                                           vp, ctypes.c_int]),
    }
    # MCGRAPH_LIB_PARTIAL=1 (A/B scripts only): an older variant library may lack newer entry points
    partial = os.environ.get("MCGRAPH_LIB_PARTIAL") == "1"
    for name, (res, args) in sig.items():
        if partial and not hasattr(L, name):
            continue
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    _lib = L
    return L


def comm_unique_id() -> bytes:
    """mc_comm_unique_id (ncclGetUniqueId): made on one rank, broadcast to the others."""
    buf = ctypes.create_string_buffer(MC_COMM_ID_BYTES)
    rc = load().mc_comm_unique_id(buf)
    if rc != MC_OK:
        raise McError(rc, "mc_comm_unique_id failed (RCCL not loadable?)")
    return buf.raw


def _ptr(a):
    return None if a is None else ctypes.c_void_p(a.ctypes.data)


def setorder_replay(level_sizes, edge_off, edge_a, edge_b, pt_off, pts, threads=0, labels=False):
    """mc_setorder_replay (host only, no device): the reference's container orders of a clustering run
    (include/mcgraph.h).  Returns dict(mask_off, mask_order, pt_off, pts, son_off, son_order[, labels])."""
    L = load()
    T = len(level_sizes)
    sz = np.ascontiguousarray(level_sizes, np.int32)
    eo = np.ascontiguousarray(edge_off, np.int64)
    ea = np.ascontiguousarray(edge_a, np.int32)
    eb = np.ascontiguousarray(edge_b, np.int32)
    po = np.ascontiguousarray(pt_off, np.int64)
    pp = np.ascontiguousarray(pts, np.int32)
    N0, NL = int(sz[0]), int(sz[T - 1])
    K = ctypes.c_int32()
    mo, mord = np.zeros(NL + 1, np.int64), np.zeros(max(N0, 1), np.int32)
    oo, opts = np.zeros(NL + 1, np.int64), np.zeros(max(int(po[N0]), 1), np.int32)
    so, sord = np.zeros(NL + 1, np.int64), np.zeros(max(NL, 1), np.int32)
    lab = np.zeros(max(int(sz.sum()), 1), np.int32) if labels else None
    rc = L.mc_setorder_replay(T, _ptr(sz), _ptr(eo), _ptr(ea), _ptr(eb), _ptr(po), _ptr(pp), int(threads),
                              ctypes.byref(K), _ptr(mo), _ptr(mord), _ptr(oo), _ptr(opts), _ptr(so), _ptr(sord),
                              _ptr(lab))
    if rc != MC_OK:
        raise McError(rc, "mc_setorder_replay: inconsistent levels / edges / point sets")
    k = K.value
    out = dict(mask_off=mo[:k + 1], mask_order=mord[:N0], pt_off=oo[:k + 1], pts=opts[:int(oo[k])],
               son_off=so[:k + 1], son_order=sord[:NL])
    if labels:
        out["labels"] = lab[:int(sz.sum())]
    return out


class SetOrder:
    """mc_setorder_begin / mc_setorder_finish: the level-0 point sets (node i: pts[node_start[i] :
    node_start[i] + node_len[i]], added in order) built on a native background thread from
    construction on, the iterations replayed by finish (the result of setorder_replay)."""

    def __init__(self, node_start, node_len, pts, threads=0, async_build=True):
        self.L = load()
        st = np.ascontiguousarray(node_start, np.int64)
        ln = np.ascontiguousarray(node_len, np.int64)
        pp = np.ascontiguousarray(pts, np.int32)
        if len(st) != len(ln) or (len(ln) and int((st + ln).max()) > len(pp)):
            raise ValueError("node ranges outside pts")
        self._keep = (st, ln, pp)  # read by the background thread until finish / close
        self.n0, self.total = len(st), int(ln.sum())
        h = ctypes.c_void_p()
        rc = self.L.mc_setorder_begin(self.n0, _ptr(st), _ptr(ln), _ptr(pp), int(threads), 1 if async_build else 0,
                                      ctypes.byref(h))
        if rc != MC_OK:
            raise McError(rc, "mc_setorder_begin: invalid node ranges / point ids")
        self.h = h

    def finish(self, level_sizes, edge_off, edge_a, edge_b, labels=False):
        if not getattr(self, "h", None):
            raise RuntimeError("SetOrder already finished")
        T = len(level_sizes)
        sz = np.ascontiguousarray(level_sizes, np.int32)
        eo = np.ascontiguousarray(edge_off, np.int64)
        ea = np.ascontiguousarray(edge_a, np.int32)
        eb = np.ascontiguousarray(edge_b, np.int32)
        N0, NL = int(sz[0]), int(sz[T - 1])
        K = ctypes.c_int32()
        mo, mord = np.zeros(NL + 1, np.int64), np.zeros(max(N0, 1), np.int32)
        oo, opts = np.zeros(NL + 1, np.int64), np.zeros(max(self.total, 1), np.int32)
        so, sord = np.zeros(NL + 1, np.int64), np.zeros(max(NL, 1), np.int32)
        lab = np.zeros(max(int(sz.sum()), 1), np.int32) if labels else None
        try:
            rc = self.L.mc_setorder_finish(self.h, T, _ptr(sz), _ptr(eo), _ptr(ea), _ptr(eb), ctypes.byref(K), _ptr(mo),
                                           _ptr(mord), _ptr(oo), _ptr(opts), _ptr(so), _ptr(sord), _ptr(lab))
        finally:
            self.close()
        if rc != MC_OK:
            raise McError(rc, "mc_setorder_finish: inconsistent levels / edges, or a negative point id")
        k = K.value
        out = dict(mask_off=mo[:k + 1], mask_order=mord[:N0], pt_off=oo[:k + 1], pts=opts[:int(oo[k])],
                   son_off=so[:k + 1], son_order=sord[:NL])
        if labels:
            out["labels"] = lab[:int(sz.sum())]
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.mc_setorder_free(self.h)
            self.h = None
        self._keep = None

    def __del__(self):
        self.close()


class Context:
    """One libmcgraph context (device memory + stream) — one scene at a time."""

    def __init__(self, device: int = 0):
        self.device_index = int(device)
        self.L = load()
        h = ctypes.c_void_p()
        rc = self.L.mc_ctx_create(int(device), ctypes.byref(h))
        if rc != MC_OK:
            raise McError(rc, "mc_ctx_create failed (no HIP device?)")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.mc_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != MC_OK:
            raise McError(rc, self.L.mc_ctx_last_error(self.h).decode())

    # ---- context ----
    def set_stream(self, stream_handle):
        self._check(self.L.mc_ctx_set_stream(self.h, ctypes.c_void_p(stream_handle) if stream_handle else None))

    def stream(self):
        return self.L.mc_ctx_get_stream(self.h)

    def synchronize(self):
        self._check(self.L.mc_ctx_synchronize(self.h))

    def set_timing(self, on: bool):
        self._check(self.L.mc_ctx_set_timing(self.h, 1 if on else 0))

    def set_timing_filter(self, name):
        self._check(self.L.mc_ctx_set_timing_filter(self.h, name.encode() if name else None))

    def kernel_time(self, name: str):
        ms, n = ctypes.c_double(), ctypes.c_int64()
        self._check(self.L.mc_ctx_get_kernel_time(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def reset_kernel_times(self):
        self._check(self.L.mc_ctx_reset_kernel_times(self.h))

    def set_memory_budget(self, nbytes: int):
        """mc_ctx_set_memory_budget: HBM bytes S1's per-batch arrays may take (0 = the default share)."""
        self._check(self.L.mc_ctx_set_memory_budget(self.h, int(nbytes)))

    def debug_counters(self, reset: bool = False):
        """(checks compiled in, failures per check kind): the in-kernel invariant checks of a
        -DMC_DBG_CHECK=1 build (docs/experiments.md); a normal build reports (False, zeros)."""
        out = np.zeros(9, np.int64)
        self._check(self.L.mc_debug_counters(self.h, _ptr(out), 9, 1 if reset else 0))
        return bool(out[0]), out[1:]

    # ---- row-block sharding over processes (include/mcgraph.h) ----
    @property
    def torch_device(self):
        import torch
        return torch.device("cuda", self.device_index)

    def shard_set(self, rank, world):
        self._check(self.L.mc_shard_set(self.h, int(rank), int(world)))

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        """mc_ctx_comm_init: an RCCL communicator owned by the context (rank / world of the sharded
        graph stages come from it; the exchanges then run inside mc_graph_build / mc_cluster_run)."""
        assert len(unique_id) == MC_COMM_ID_BYTES
        buf = ctypes.create_string_buffer(bytes(unique_id), MC_COMM_ID_BYTES)
        self._check(self.L.mc_ctx_comm_init(self.h, buf, int(rank), int(world)))

    def attach_comm(self, nccl_comm):
        """mc_ctx_attach_comm: a caller-owned ncclComm_t (an int address); None detaches."""
        self._check(self.L.mc_ctx_attach_comm(self.h, None if nccl_comm is None else ctypes.c_void_p(int(nccl_comm))))

    def shard_pending(self) -> int:
        ph = ctypes.c_int32()
        self._check(self.L.mc_shard_pending(self.h, ctypes.byref(ph)))
        return ph.value

    def shard_export_size(self, phase) -> int:
        n = ctypes.c_int64()
        self._check(self.L.mc_shard_export(self.h, int(phase), None, ctypes.byref(n)))
        return n.value

    def shard_export(self, phase, out):
        """this rank's block into the device tensor ``out`` (stream-ordered on the context stream)"""
        n = ctypes.c_int64()
        self._check(self.L.mc_shard_export(self.h, int(phase), ctypes.c_void_p(out.data_ptr()), ctypes.byref(n)))

    def shard_import(self, phase, blocks, stride_bytes):
        """every rank's block ([world][stride_bytes] in rank order; HIST: the summed block)"""
        self._check(self.L.mc_shard_import(self.h, int(phase), ctypes.c_void_p(blocks.data_ptr()), int(stride_bytes)))

    # ---- scene ----
    def set_masks(self, num_points, num_frames, mask_col, mask_label, mask_off, mask_pts=None, pts_device_ptr=None):
        col = np.ascontiguousarray(mask_col, np.int32)
        lab = np.ascontiguousarray(mask_label, np.int32)
        off = np.ascontiguousarray(mask_off, np.int64)
        if pts_device_ptr is not None:
            pts_p, on_dev = ctypes.c_void_p(int(pts_device_ptr)), 1
        else:
            pts = np.ascontiguousarray(mask_pts, np.int32)
            self._keep_pts = pts
            pts_p, on_dev = _ptr(pts), 0
        self._check(self.L.mc_scene_set_masks(self.h, int(num_points), int(num_frames), len(col), _ptr(col),
                                               _ptr(lab), _ptr(off), pts_p, on_dev))

    def build(self, mask_visible_threshold, contained_threshold, undersegment_filter_threshold):
        prm = GraphParams(float(mask_visible_threshold), float(contained_threshold),
                          float(undersegment_filter_threshold))
        self._check(self.L.mc_graph_build(self.h, ctypes.byref(prm)))

    def graph_info(self) -> GraphInfo:
        info = GraphInfo()
        self._check(self.L.mc_graph_get_info(self.h, ctypes.byref(info)))
        return info

    def global_masks(self, M):
        out = np.zeros(max(M, 1), np.int32)
        self._check(self.L.mc_graph_get_global_masks(self.h, _ptr(out)))
        return out[:M]

    def boundary(self, P):
        out = np.zeros(max(P, 1), np.uint8)
        self._check(self.L.mc_graph_get_boundary(self.h, _ptr(out)))
        return out[:P]

    def point_in_mask(self, P, F):
        out = np.zeros((max(P, 1), max(F, 1)), np.uint16)
        self._check(self.L.mc_graph_get_point_in_mask(self.h, _ptr(out)))
        return out[:P, :F]

    def point_frame_bits(self, P, F):
        FW = (F + 63) // 64
        out = np.zeros((max(P, 1), max(FW, 1)), np.uint64)
        self._check(self.L.mc_graph_get_point_frame_bits(self.h, _ptr(out)))
        return out[:P, :FW]

    def visible_frame_bits(self, M, F):
        FW = (F + 63) // 64
        out = np.zeros((max(M, 1), max(FW, 1)), np.uint64)
        self._check(self.L.mc_graph_get_visible_frame_bits(self.h, _ptr(out)))
        return out[:M, :FW]

    def contained(self, M, nnz):
        off = np.zeros(M + 1, np.int64)
        idx = np.zeros(max(nnz, 1), np.int32)
        self._check(self.L.mc_graph_get_contained(self.h, _ptr(off), _ptr(idx)))
        return off, idx[:nnz]

    def undersegment(self, n):
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.L.mc_graph_get_undersegment(self.h, _ptr(out)))
        return out[:n]

    def nodes0(self, n):
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.L.mc_graph_get_nodes0(self.h, _ptr(out)))
        return out[:n]

    def observer_hist(self, F):
        out = np.zeros(F + 1, np.uint64)
        self._check(self.L.mc_graph_get_observer_hist(self.h, _ptr(out)))
        return out

    def thresholds(self):
        thr = np.zeros(20, np.float32)
        isint = np.zeros(20, np.int32)
        n = ctypes.c_int32()
        self._check(self.L.mc_graph_get_thresholds(self.h, _ptr(thr), _ptr(isint), ctypes.byref(n)))
        return thr[:n.value].copy(), isint[:n.value].astype(bool)

    def observer_thresholds(self, vf_bits, num_frames):
        """get_observer_num_thresholds (construction.py:80-96) on explicit VF bit rows."""
        vf = np.ascontiguousarray(vf_bits, np.uint64)
        thr = np.zeros(20, np.float32)
        isint = np.zeros(20, np.int32)
        n = ctypes.c_int32()
        self._check(self.L.mc_observer_thresholds(self.h, vf.shape[0], int(num_frames), _ptr(vf), _ptr(thr),
                                                  _ptr(isint), ctypes.byref(n)))
        return thr[:n.value].copy(), isint[:n.value].astype(bool)

    # ---- nodes / clustering ----
    def set_nodes(self, num_frames, num_masks, num_points, vf_bits, c_off, c_idx, pt_off, pt_idx):
        vf = np.ascontiguousarray(vf_bits, np.uint64)
        c_off = np.ascontiguousarray(c_off, np.int64)
        c_idx = np.ascontiguousarray(c_idx, np.int32)
        pt_off = np.ascontiguousarray(pt_off, np.int64)
        pt_idx = np.ascontiguousarray(pt_idx, np.int32)
        n = len(c_off) - 1
        self._check(self.L.mc_nodes_set(self.h, n, int(num_frames), int(num_masks), int(num_points), _ptr(vf),
                                        _ptr(c_off), _ptr(c_idx), _ptr(pt_off), _ptr(pt_idx)))

    def cluster(self, thresholds, connect_threshold):
        if thresholds is None:
            self._check(self.L.mc_cluster_run(self.h, None, 0, float(connect_threshold)))
        else:
            thr = np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32))
            self._check(self.L.mc_cluster_run(self.h, _ptr(thr), len(thr), float(connect_threshold)))

    def cluster_info(self) -> ClusterInfo:
        info = ClusterInfo()
        self._check(self.L.mc_cluster_get_info(self.h, ctypes.byref(info)))
        return info

    def level_sizes(self, n_iter):
        out = np.zeros(n_iter + 1, np.int32)
        self._check(self.L.mc_cluster_get_level_sizes(self.h, _ptr(out)))
        return out

    def set_edge_capture(self, capacity):
        self._check(self.L.mc_cluster_set_edge_capture(self.h, int(capacity)))

    def edges(self):
        """captured edges as (t, a, b) int64 arrays, sorted by (t, a, b)"""
        n = ctypes.c_int64()
        self._check(self.L.mc_cluster_get_edges(self.h, None, ctypes.byref(n)))
        keys = np.zeros(max(n.value, 1), np.uint64)
        self._check(self.L.mc_cluster_get_edges(self.h, _ptr(keys), ctypes.byref(n)))
        keys = np.sort(keys[:n.value])
        return ((keys >> np.uint64(48)).astype(np.int64), ((keys >> np.uint64(24)) & np.uint64(0xffffff)).astype(np.int64),
                (keys & np.uint64(0xffffff)).astype(np.int64))

    def level_caps(self, n_iter):
        out = np.zeros(n_iter + 1, np.int32)
        self._check(self.L.mc_cluster_get_level_caps(self.h, _ptr(out)))
        return out

    def partition(self, t, n):
        out = np.zeros(max(n, 1), np.int32)
        self._check(self.L.mc_cluster_get_partition(self.h, int(t), _ptr(out)))
        return out[:n]

    def edge_counts(self, n_iter):
        out = np.zeros(max(n_iter, 1), np.int64)
        self._check(self.L.mc_cluster_get_edge_counts(self.h, _ptr(out)))
        return out[:n_iter]

    def final_labels(self, n0):
        out = np.zeros(max(n0, 1), np.int32)
        self._check(self.L.mc_cluster_get_final_labels(self.h, _ptr(out)))
        return out[:n0]

    def objects(self, info: ClusterInfo, F):
        K = info.num_objects
        FW = (F + 63) // 64
        vf = np.zeros((max(K, 1), max(FW, 1)), np.uint64)
        c_off = np.zeros(K + 1, np.int64)
        c_idx = np.zeros(max(info.num_object_contained, 1), np.int32)
        pt_off = np.zeros(K + 1, np.int64)
        pt_idx = np.zeros(max(info.num_object_points, 1), np.int32)
        m_off = np.zeros(K + 1, np.int64)
        m_idx = np.zeros(max(info.num_object_masks, 1), np.int32)
        self._check(self.L.mc_cluster_get_objects(self.h, _ptr(vf), _ptr(c_off), _ptr(c_idx), _ptr(pt_off),
                                                  _ptr(pt_idx), _ptr(m_off), _ptr(m_idx)))
        return dict(vf_bits=vf[:K, :FW], c_off=c_off, c_idx=c_idx[:c_off[-1]], pt_off=pt_off,
                    pt_idx=pt_idx[:pt_off[-1]], mask_off=m_off, mask_idx=m_idx[:m_off[-1]])


def bp_params(**kw) -> BpParams:
    """The reference's S1 constants, with optional overrides."""
    p = BpParams()
    load().mc_bp_params_default(ctypes.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _bp_methods():
    def set_points(self, xyz=None, device_ptr=None, num_points=None):
        """Scene points as float32 [P,3] (construction.py:37 casts them to float32)."""
        if device_ptr is not None:
            self._check(self.L.mc_scene_set_points(self.h, int(num_points), ctypes.c_void_p(int(device_ptr)), 1))
            return
        pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        self._check(self.L.mc_scene_set_points(self.h, len(pts), _ptr(pts), 0))

    def backproject(self, depth, seg, intrinsics, poses, params: BpParams | None = None, device_ptrs=None,
                    shape=None):
        """S1 for a batch of frames: depth float32 [F,H,W], seg uint8 [F,H,W], intrinsics [F,4],
        poses [F,4,4].  device_ptrs = (depth, seg, intrinsics, poses) device pointers with shape=(F,H,W)."""
        prm = params or bp_params()
        if device_ptrs is not None:
            F, H, W = shape
            d, s_, k, t = (ctypes.c_void_p(int(x)) for x in device_ptrs)
            self._check(self.L.mc_backproject(self.h, F, H, W, d, s_, k, t, 1, ctypes.byref(prm)))
            return
        depth = np.ascontiguousarray(depth, np.float32)
        seg = np.ascontiguousarray(seg, np.uint8)
        F, H, W = depth.shape
        assert seg.shape == depth.shape
        K = np.ascontiguousarray(intrinsics, np.float64).reshape(F, 4)
        T = np.ascontiguousarray(poses, np.float64).reshape(F, 16)
        self._check(self.L.mc_backproject(self.h, F, H, W, _ptr(depth), _ptr(seg), _ptr(K), _ptr(T), 0,
                                          ctypes.byref(prm)))

    def backproject_frames(self, depth_frames, seg_frames, intrinsics, poses, params: BpParams | None = None,
                           depth_scale=None):
        """S1 from per-frame host arrays (depth float32 [H,W], seg uint8 [H,W] each, C-contiguous),
        staged to the device without an [F,H,W] host copy (mc_backproject_frames).  With
        depth_scale, the depth frames are the PNGs' uint16 values, decoded on the device
        (mc_backproject_frames_raw)."""
        prm = params or bp_params()
        F = len(depth_frames)
        assert len(seg_frames) == F and F > 0
        H, W = depth_frames[0].shape
        dt = np.float32 if depth_scale is None else np.uint16
        for d, sg in zip(depth_frames, seg_frames):
            if d.shape != (H, W) or sg.shape != (H, W) or d.dtype != dt or sg.dtype != np.uint8 \
                    or not d.flags.c_contiguous or not sg.flags.c_contiguous:
                raise ValueError(f"frames must be C-contiguous {np.dtype(dt).name} depth / uint8 seg arrays of one shape")
        dp = (ctypes.c_void_p * F)(*[d.ctypes.data for d in depth_frames])
        sp = (ctypes.c_void_p * F)(*[sg.ctypes.data for sg in seg_frames])
        K = np.ascontiguousarray(intrinsics, np.float64).reshape(F, 4)
        T = np.ascontiguousarray(poses, np.float64).reshape(F, 16)
        if depth_scale is None:
            self._check(self.L.mc_backproject_frames(self.h, F, H, W, dp, sp, _ptr(K), _ptr(T), ctypes.byref(prm)))
        else:
            self._check(self.L.mc_backproject_frames_raw(self.h, F, H, W, dp, float(depth_scale), sp, _ptr(K), _ptr(T),
                                                         ctypes.byref(prm)))

    def bp_info(self) -> BpInfo:
        info = BpInfo()
        self._check(self.L.mc_backproject_get_info(self.h, ctypes.byref(info)))
        return info

    def bp_batching(self) -> dict:
        """mc_backproject_get_batching: S1's frames per batch (last call), mask-pixel capacity, the
        bytes the per-batch arrays hold, and the batches redone after a mask-pixel overflow."""
        out = np.zeros(4, np.int64)
        self._check(self.L.mc_backproject_get_batching(self.h, _ptr(out)))
        return dict(frames_per_batch=int(out[0]), mask_pixel_cap=int(out[1]), bytes_held=int(out[2]),
                    redone=int(out[3]))

    def bp_masks(self):
        info = self.bp_info()
        M = info.num_masks
        col = np.zeros(max(M, 1), np.int32)
        lab = np.zeros(max(M, 1), np.int32)
        off = np.zeros(M + 1, np.int64)
        pts = np.zeros(max(info.num_mask_points, 1), np.int32)
        self._check(self.L.mc_backproject_get_masks(self.h, _ptr(col), _ptr(lab), _ptr(off), _ptr(pts)))
        return col[:M], lab[:M], off, pts[:info.num_mask_points]

    def bp_mask_index(self):
        """(mask_col, mask_label, mask_off) of the back-projected masks, without the point lists."""
        M = self.bp_info().num_masks
        col = np.zeros(max(M, 1), np.int32)
        lab = np.zeros(max(M, 1), np.int32)
        off = np.zeros(M + 1, np.int64)
        self._check(self.L.mc_backproject_get_masks(self.h, _ptr(col), _ptr(lab), _ptr(off), None))
        return col[:M], lab[:M], off

    def bp_points_to_device(self, dst_ptr):
        """Stream-ordered device-to-device copy of the mask point lists (int32) to dst_ptr."""
        self._check(self.L.mc_backproject_copy_points_device(self.h, ctypes.c_void_p(int(dst_ptr))))

    def bp_candidates(self):
        n = self.bp_info().num_candidates
        st = np.zeros((max(n, 1), MC_BP_NSTAT), np.int32)
        self._check(self.L.mc_backproject_get_candidates(self.h, _ptr(st)))
        return st[:n]

    def bp_voxels(self) -> dict:
        """mc_backproject_get_voxels: the pixel lists and voxel means of the last call's slots (a call of one
        batch), in candidate order: slots [NS,4] (frame, id, pixels, voxels), pixels / means / origin as
        per-slot lists, handed = (slots the first voxel tier handed on, slots the second did)."""
        sizes = np.zeros(3, np.int64)
        self._check(self.L.mc_backproject_get_voxels(self.h, _ptr(sizes), None, None, None, None, None))
        ns, npx, nvx = (int(x) for x in sizes)
        slots = np.zeros((max(ns, 1), 4), np.int32)
        pix = np.zeros(max(npx, 1), np.uint32)
        means = np.zeros((max(nvx, 1), 3), np.float64)
        origin = np.zeros((max(ns, 1), 3), np.float64)
        handed = np.zeros(2, np.int32)
        self._check(self.L.mc_backproject_get_voxels(self.h, _ptr(sizes), _ptr(slots), _ptr(pix), _ptr(means),
                                                     _ptr(origin), _ptr(handed)))
        slots = slots[:ns]
        po = np.concatenate([[0], np.cumsum(slots[:, 2], dtype=np.int64)])
        vo = np.concatenate([[0], np.cumsum(slots[:, 3], dtype=np.int64)])
        return dict(slots=slots, pixels=[pix[po[i]:po[i + 1]] for i in range(ns)],
                    means=[means[vo[i]:vo[i + 1]] for i in range(ns)], origin=origin[:ns],
                    handed=(int(handed[0]), int(handed[1])))

    def use_backprojection(self):
        self._check(self.L.mc_scene_use_backprojection(self.h))

    for f in (set_points, backproject, backproject_frames, bp_info, bp_batching, bp_masks, bp_mask_index,
              bp_points_to_device, bp_candidates, bp_voxels, use_backprojection):
        setattr(Context, f.__name__, f)


_bp_methods()


def _pp_methods():
    def pp_run(self, params: PPParams, scene_xyz, pfm_bits, num_frames, mask_off, mask_pts, node_vf_bits,
               node_pt_off, node_pts, node_mask_off, node_masks, node_mask_col):
        a = dict(scene=np.ascontiguousarray(scene_xyz, np.float64), pfm=np.ascontiguousarray(pfm_bits, np.uint64),
                 moff=np.ascontiguousarray(mask_off, np.int64), mpts=np.ascontiguousarray(mask_pts, np.int32),
                 vf=np.ascontiguousarray(node_vf_bits, np.uint64), poff=np.ascontiguousarray(node_pt_off, np.int64),
                 pts=np.ascontiguousarray(node_pts, np.int32), qoff=np.ascontiguousarray(node_mask_off, np.int64),
                 qm=np.ascontiguousarray(node_masks, np.int32), qc=np.ascontiguousarray(node_mask_col, np.int32))
        self._pp_points = a["scene"].shape[0]
        self._check(self.L.mc_pp_run(self.h, ctypes.byref(params), a["scene"].shape[0], int(num_frames), _ptr(a["scene"]),
                                     _ptr(a["pfm"]), len(a["moff"]) - 1, _ptr(a["moff"]), _ptr(a["mpts"]),
                                     len(a["poff"]) - 1, _ptr(a["vf"]), _ptr(a["poff"]), _ptr(a["pts"]), _ptr(a["qoff"]),
                                     _ptr(a["qm"]), _ptr(a["qc"])))

    def pp_info(self) -> PPInfo:
        info = PPInfo()
        self._check(self.L.mc_pp_get_info(self.h, ctypes.byref(info)))
        return info

    def pp_results(self):
        i = self.pp_info()
        K, E, Q = i.num_objects, i.num_entries, i.num_node_masks
        r = dict(entry_object=np.zeros(max(E, 1), np.int32), mask_object=np.zeros(max(Q, 1), np.int32),
                 mask_coverage=np.zeros(max(Q, 1), np.float64), object_state=np.zeros(max(K, 1), np.uint8),
                 object_node=np.zeros(max(K, 1), np.int32), object_bbox=np.zeros((max(K, 1), 6), np.float64))
        self._check(self.L.mc_pp_get_results(self.h, _ptr(r["entry_object"]), _ptr(r["mask_object"]),
                                             _ptr(r["mask_coverage"]), _ptr(r["object_state"]), _ptr(r["object_node"]),
                                             _ptr(r["object_bbox"])))
        n = dict(entry_object=E, mask_object=Q, mask_coverage=Q, object_state=K, object_node=K, object_bbox=K)
        return {k: v[:n[k]] for k, v in r.items()}

    def _dptr(t):
        return None if t is None or t.numel() == 0 else ctypes.c_void_p(t.data_ptr())

    def pp_run_device(self, params: PPParams, scene_xyz, pfm_bits, num_frames, mask_off, mask_pts, node_vf_bits,
                      node_pt_off, node_pts, node_mask_off, node_masks, node_mask_col):
        """mc_pp_run_device: the arguments of pp_run as contiguous device tensors (scene f64 [P,3], bit
        rows as int64/uint64 words, offsets int64, indices int32)."""
        import torch
        want = dict(scene=torch.float64, moff=torch.int64, mpts=torch.int32, poff=torch.int64, pts=torch.int32,
                    qoff=torch.int64, qm=torch.int32, qc=torch.int32)
        a = dict(scene=scene_xyz, pfm=pfm_bits, moff=mask_off, mpts=mask_pts, vf=node_vf_bits, poff=node_pt_off,
                 pts=node_pts, qoff=node_mask_off, qm=node_masks, qc=node_mask_col)
        for k, t in a.items():
            if t.device.type != "cuda" or not t.is_contiguous() or (k in want and t.dtype != want[k]) or \
                    (k in ("pfm", "vf") and t.element_size() != 8):
                raise ValueError(f"pp_run_device: {k} must be a contiguous device tensor of the documented type")
        off = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731  (offsets hold at least one entry)
        self._pp_points = a["scene"].shape[0]
        self._check(self.L.mc_pp_run_device(self.h, ctypes.byref(params), a["scene"].shape[0], int(num_frames),
                                            _dptr(a["scene"]), _dptr(a["pfm"]), len(a["moff"]) - 1, off(a["moff"]),
                                            _dptr(a["mpts"]), len(a["poff"]) - 1, _dptr(a["vf"]), off(a["poff"]),
                                            _dptr(a["pts"]), off(a["qoff"]), _dptr(a["qm"]), _dptr(a["qc"])))

    def pp_run_clustered(self, params: PPParams, scene_xyz=None):
        """mc_pp_run_clustered on the context's S1-S6 result.  scene_xyz: None (the float32 points of
        set_points, widened), a float64 [P,3] numpy array, or a contiguous float64 device tensor."""
        if scene_xyz is None:
            ptr, dev, keep = None, 0, None
        elif hasattr(scene_xyz, "data_ptr"):
            import torch
            if scene_xyz.device.type != "cuda" or scene_xyz.dtype != torch.float64 or not scene_xyz.is_contiguous():
                raise ValueError("pp_run_clustered: a device scene must be a contiguous float64 tensor")
            ptr, dev, keep = ctypes.c_void_p(scene_xyz.data_ptr()), 1, scene_xyz
        else:
            keep = np.ascontiguousarray(scene_xyz, np.float64)
            ptr, dev = _ptr(keep), 0
        self._check(self.L.mc_pp_run_clustered(self.h, ctypes.byref(params), ptr, dev))
        self._pp_points = int(self.graph_info().num_points)

    def pp_export_sizes(self):
        nf, npt, nm = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.L.mc_pp_export_info(self.h, ctypes.byref(nf), ctypes.byref(npt), ctypes.byref(nm)))
        return nf.value, npt.value, nm.value

    def pp_export(self, device: bool = False):
        """mc_pp_export: dict of obj_pt_off, obj_pts, obj_mask_off, obj_masks, obj_mask_cov, obj_repre
        [num_final, 5] and obj_node: numpy arrays, or tensors on the context's device."""
        nf, npt, nm = self.pp_export_sizes()
        shapes = dict(obj_pt_off=(nf + 1, "int64"), obj_pts=(npt, "int32"), obj_mask_off=(nf + 1, "int64"),
                      obj_masks=(nm, "int32"), obj_mask_cov=(nm, "float64"), obj_repre=(nf * 5, "int32"),
                      obj_node=(nf, "int32"))
        if device:
            import torch
            r = {k: torch.zeros(max(n, 1), dtype=getattr(torch, dt), device=self.torch_device)
                 for k, (n, dt) in shapes.items()}
            p = [ctypes.c_void_p(r[k].data_ptr()) for k in shapes]
        else:
            r = {k: np.zeros(max(n, 1), dt) for k, (n, dt) in shapes.items()}
            p = [_ptr(r[k]) for k in shapes]
        self._check(self.L.mc_pp_export(self.h, *p, 1 if device else 0))
        r = {k: v[:shapes[k][0]] for k, v in r.items()}
        r["obj_repre"] = r["obj_repre"].reshape(nf, 5)
        return r

    def pp_pred_masks(self, num_points: int | None = None, device: bool = False):
        """mc_pp_export_pred_masks: the [P, num_final] uint8 matrix of the prediction npz (P: the
        scene of the last pp_run* call of this object when not given)."""
        nf = self.pp_export_sizes()[0]
        if num_points is None:
            num_points = self._pp_points
        n = int(num_points) * nf
        if device:
            import torch
            out = torch.zeros(max(n, 1), dtype=torch.uint8, device=self.torch_device)
            p = ctypes.c_void_p(out.data_ptr())
        else:
            out = np.zeros(max(n, 1), np.uint8)
            p = _ptr(out)
        self._check(self.L.mc_pp_export_pred_masks(self.h, p, 1 if device else 0))
        return out[:n].reshape(int(num_points), nf)

    for f in (pp_run, pp_info, pp_results, pp_run_device, pp_run_clustered, pp_export_sizes, pp_export, pp_pred_masks):
        setattr(Context, f.__name__, f)


_pp_methods()


def _eval_methods():
    def eval_match_counts(self, pred_masks, gt_instance, num_gt, void_flags):
        """evaluation/evaluate.py:289-308 on the device: (vert counts [K], void intersections [K],
        intersections [K, num_gt]) of the columns of pred_masks [P, K]."""
        pm = np.ascontiguousarray(np.asarray(pred_masks) != 0, np.uint8)
        P, K = pm.shape
        g = np.ascontiguousarray(gt_instance, np.int32)
        v = np.ascontiguousarray(void_flags, np.uint8)
        verts, vint = np.zeros(max(K, 1), np.int64), np.zeros(max(K, 1), np.int64)
        inter = np.zeros((max(K, 1), max(int(num_gt), 1)), np.int64)
        self._check(self.L.mc_eval_match_counts(self.h, P, K, _ptr(pm), _ptr(g), int(num_gt), _ptr(v), _ptr(verts),
                                                _ptr(vint), _ptr(inter)))
        return verts[:K], vint[:K], inter[:K, :int(num_gt)]

    Context.eval_match_counts = eval_match_counts


_eval_methods()


EV_TABLE_KEYS = (("gt_cls", "int32"), ("gt_id", "int32"), ("gt_vert", "int64"), ("pr_cls", "int32"), ("pr_vert", "int64"),
                 ("pr_void", "int64"), ("pr_score", "float64"), ("pair_pred", "int32"), ("pair_gt", "int32"),
                 ("pair_int", "int64"))


def _ev_methods():
    def ev_begin(self, class_ids, overlaps=None, min_region_size=100, no_class=False):
        """mc_ev_begin: start or reset the AP accumulation.  overlaps default to the reference's
        (evaluate.py:44), passed as the doubles numpy computed."""
        ids = np.ascontiguousarray(class_ids, np.int32)
        ov = np.ascontiguousarray(np.append(np.arange(0.5, 0.95, 0.05), 0.25) if overlaps is None else overlaps, np.float64)
        self._check(self.L.mc_ev_begin(self.h, len(ids), _ptr(ids), len(ov), _ptr(ov), int(min_region_size),
                                       1 if no_class else 0))
        self._ev_shape = (len(ids), len(ov))

    def ev_add_scan(self, gt_ids, pred_off, pred_pts, pred_classes=None, pred_scores=None):
        """mc_ev_add_scan: ground-truth ids [P] and predictions as point lists (CSR): numpy arrays, or
        contiguous tensors on the context's device (int32 / int64 / float64 as in the header), all of one kind."""
        dev = hasattr(gt_ids, "data_ptr")
        if dev:
            import torch
            want = (torch.int32, torch.int64, torch.int32, torch.int32, torch.float64)
            args = (gt_ids, pred_off, pred_pts, pred_classes, pred_scores)
            for a, dt in zip(args, want):
                if a is not None and (a.device.type != "cuda" or a.dtype != dt or not a.is_contiguous()):
                    raise ValueError("ev_add_scan: device inputs must be contiguous tensors of the header's types")
            p = [None if a is None else ctypes.c_void_p(a.data_ptr()) for a in args]
            P, K, n = gt_ids.numel(), pred_off.numel() - 1, pred_pts.numel()
        else:
            args = (np.ascontiguousarray(gt_ids, np.int32), np.ascontiguousarray(pred_off, np.int64),
                    np.ascontiguousarray(pred_pts, np.int32),
                    None if pred_classes is None else np.ascontiguousarray(pred_classes, np.int32),
                    None if pred_scores is None else np.ascontiguousarray(pred_scores, np.float64))
            p = [_ptr(a) for a in args]
            P, K, n = len(args[0]), len(args[1]) - 1, len(args[2])
        if K < 0:
            raise ValueError("ev_add_scan: pred_off needs at least one entry")
        self._check(self.L.mc_ev_add_scan(self.h, P, p[0], K, p[1], n, p[2], p[3], p[4], 1 if dev else 0))

    def ev_add_scan_clustered(self, gt_ids):
        """mc_ev_add_scan_clustered: the last post-processing result's final objects against gt_ids [P]
        (numpy, or an int32 tensor on the context's device)."""
        if hasattr(gt_ids, "data_ptr"):
            import torch
            if gt_ids.device.type != "cuda" or gt_ids.dtype != torch.int32 or not gt_ids.is_contiguous():
                raise ValueError("ev_add_scan_clustered: a device gt_ids must be a contiguous int32 tensor")
            n, p, dev = gt_ids.numel(), ctypes.c_void_p(gt_ids.data_ptr()), 1
        else:
            keep = np.ascontiguousarray(gt_ids, np.int32)
            n, p, dev = len(keep), _ptr(keep), 0
        if getattr(self, "_pp_points", None) is not None and n != self._pp_points:
            raise ValueError(f"ev_add_scan_clustered: {n} ground-truth ids for a scene of {self._pp_points} points")
        self._check(self.L.mc_ev_add_scan_clustered(self.h, p, dev))

    def ev_add_matches(self, tables):
        """mc_ev_add_matches: a scan as its tables (dict with the keys of ``ev_scan``)."""
        a = {k: np.ascontiguousarray(tables[k], dt) for k, dt in EV_TABLE_KEYS}
        if not (len(a["gt_cls"]) == len(a["gt_id"]) == len(a["gt_vert"]) and
                len(a["pr_cls"]) == len(a["pr_vert"]) == len(a["pr_void"]) == len(a["pr_score"]) and
                len(a["pair_pred"]) == len(a["pair_gt"]) == len(a["pair_int"])):
            raise ValueError("ev_add_matches: table columns differ in length")
        self._check(self.L.mc_ev_add_matches(self.h, len(a["gt_cls"]), _ptr(a["gt_cls"]), _ptr(a["gt_id"]), _ptr(a["gt_vert"]),
                                             len(a["pr_cls"]), _ptr(a["pr_cls"]), _ptr(a["pr_vert"]), _ptr(a["pr_void"]),
                                             _ptr(a["pr_score"]), len(a["pair_pred"]), _ptr(a["pair_pred"]),
                                             _ptr(a["pair_gt"]), _ptr(a["pair_int"])))

    def ev_scan(self):
        """mc_ev_scan_info + mc_ev_get_scan: the last added scan's tables."""
        g, k, n = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int64(0)
        self._check(self.L.mc_ev_scan_info(self.h, ctypes.byref(g), ctypes.byref(k), ctypes.byref(n)))
        size = {"gt": g.value, "pr": k.value, "pa": n.value}
        r = {key: np.zeros(max(size[key[:2]], 1), dt) for key, dt in EV_TABLE_KEYS}
        self._check(self.L.mc_ev_get_scan(self.h, *[_ptr(r[key]) for key, _ in EV_TABLE_KEYS]))
        return {key: r[key][:size[key[:2]]] for key, _ in EV_TABLE_KEYS}

    def ev_ap(self):
        """mc_ev_ap: (ap [C, O], stats [C, O, 4]: examples, true examples, hard false negatives, flags)."""
        C, O = self._ev_shape
        ap, stats = np.zeros((C, O), np.float64), np.zeros((C, O, 4), np.int64)
        self._check(self.L.mc_ev_ap(self.h, _ptr(ap), _ptr(stats)))
        return ap, stats

    def ev_curve(self, class_index, overlap_index):
        """mc_ev_get_curve: (scores ascending, tp, fp, fn) of a cell, empty for a cell without a curve."""
        n = ctypes.c_int64(0)
        self._check(self.L.mc_ev_get_curve(self.h, int(class_index), int(overlap_index), ctypes.byref(n), None, None, None, None))
        sc = np.zeros(max(n.value, 1), np.float64)
        tp, fp, fn = (np.zeros(max(n.value, 1), np.int64) for _ in range(3))
        if n.value:
            self._check(self.L.mc_ev_get_curve(self.h, int(class_index), int(overlap_index), ctypes.byref(n), _ptr(sc), _ptr(tp),
                                               _ptr(fp), _ptr(fn)))
        return sc[:n.value], tp[:n.value], fp[:n.value], fn[:n.value]

    def ev_state_info(self):
        """mc_ev_state_info: (runs, examples, bytes) of the accumulation's state buffer."""
        r, e, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        self._check(self.L.mc_ev_state_info(self.h, ctypes.byref(r), ctypes.byref(e), ctypes.byref(b)))
        return r.value, e.value, b.value

    def ev_state(self, device: bool = False):
        """mc_ev_state_export: the accumulation as its state buffer (include/mcgraph.h): a uint8 numpy array,
        or with device a uint8 tensor on the context's device."""
        n = self.ev_state_info()[2]
        if device:
            import torch
            out = torch.empty(n, dtype=torch.uint8, device=self.torch_device)
            self._check(self.L.mc_ev_state_export(self.h, ctypes.c_void_p(out.data_ptr()), n, 1))
            return out
        out = np.zeros(n, np.uint8)
        self._check(self.L.mc_ev_state_export(self.h, _ptr(out), n, 0))
        return out

    def ev_merge_state(self, buf):
        """mc_ev_state_merge: add a state buffer (bytes, a uint8 numpy array or a uint8 tensor; a tensor on the
        context's device is read there) to the accumulation."""
        if hasattr(buf, "data_ptr"):
            import torch
            if buf.dtype != torch.uint8 or not buf.is_contiguous():
                raise ValueError("ev_merge_state: a tensor must be contiguous uint8")
            if buf.device.type == "cuda":
                torch.cuda.current_stream(buf.device).synchronize()   # the context reads it on its own stream
                self._check(self.L.mc_ev_state_merge(self.h, ctypes.c_void_p(buf.data_ptr()), buf.numel(), 1))
                return
            buf = buf.numpy()
        a = np.ascontiguousarray(np.frombuffer(buf, np.uint8) if isinstance(buf, (bytes, bytearray, memoryview)) else buf)
        if a.dtype != np.uint8 or a.ndim != 1:
            raise ValueError("ev_merge_state: a uint8 vector")
        self._check(self.L.mc_ev_state_merge(self.h, _ptr(a) if a.size else None, a.size, 0))

    for f in (ev_begin, ev_add_scan, ev_add_scan_clustered, ev_add_matches, ev_scan, ev_ap, ev_curve, ev_state_info, ev_state,
              ev_merge_state):
        setattr(Context, f.__name__, f)


_ev_methods()


def _ov_methods():
    def openvoc_query(self, obj_off, obj_rows, features, label_features, temperature=100.0):
        """semantics/open-voc_query.py:32-50 on the device: label index of every object (-1: none)."""
        off = np.ascontiguousarray(obj_off, np.int64)
        rows = np.ascontiguousarray(obj_rows, np.int32)
        feats = np.ascontiguousarray(features, np.float32)
        labs = np.ascontiguousarray(label_features, np.float32)
        K = len(off) - 1
        out = np.zeros(max(K, 1), np.int32)
        self._check(self.L.mc_openvoc_query(self.h, K, _ptr(off), _ptr(rows), feats.shape[0], labs.shape[1],
                                            _ptr(feats), labs.shape[0], _ptr(labs), float(temperature), _ptr(out)))
        return out[:K]

    Context.openvoc_query = openvoc_query


_ov_methods()


def _io_methods():
    def frames_decode(self, num_frames, height, width, depth_ptr, depth_scale, seg_shape, seg_ptr, on_device,
                      depth_out_ptr, seg_out_ptr):
        """mc_frames_decode (dataset/scannet.py:49-54, :68-73); pointers as ints (None = skip)."""
        c = lambda x: None if x is None else ctypes.c_void_p(int(x))
        hs, ws = seg_shape
        self._check(self.L.mc_frames_decode(self.h, int(num_frames), int(height), int(width), c(depth_ptr),
                                            float(depth_scale), int(hs), int(ws), c(seg_ptr), 1 if on_device else 0,
                                            c(depth_out_ptr), c(seg_out_ptr)))

    Context.frames_decode = frames_decode


_io_methods()


def crop_params(**kw) -> CropParams:
    """The reference's crop constants with open_clip's OpenAI mean / std, with optional overrides
    (mean, std, pad_rgb as 3-sequences)."""
    p = CropParams()
    load().mc_crop_params_default(ctypes.byref(p))
    for k, v in kw.items():
        if k in ("mean", "std", "pad_rgb"):
            v = type(getattr(p, k))(*v)
        elif not hasattr(p, k):
            raise TypeError(f"unknown crop parameter {k}")
        setattr(p, k, v)
    return p


def _crop_methods():
    def _frames(self, a, channels, name):
        """(pointer, on_device, F, H, W, keep-alive) of a uint8 frame stack: numpy or a device tensor"""
        nd = 4 if channels else 3
        if hasattr(a, "data_ptr"):
            import torch
            if a.dtype != torch.uint8 or a.dim() != nd or not a.is_contiguous() or (channels and a.shape[3] != channels):
                raise ValueError(f"{name}: a contiguous uint8 tensor [F, H, W{', 3' if channels else ''}]")
            if a.device.type == "cuda":
                return ctypes.c_void_p(a.data_ptr()), 1, a.shape[0], a.shape[1], a.shape[2], a
            a = a.numpy()
        a = np.ascontiguousarray(a)
        if a.dtype != np.uint8 or a.ndim != nd or (channels and a.shape[3] != channels):
            raise ValueError(f"{name}: a uint8 array [F, H, W{', 3' if channels else ''}]")
        return _ptr(a), 0, a.shape[0], a.shape[1], a.shape[2], a

    def _order(self):
        """Device tensors live on torch's current stream, the kernels run on the context's.  When the two
        differ the host waits for torch's stream before the call and (True returned) for the context's
        after it; when the context runs on torch's stream (set_stream) nothing waits."""
        import torch
        cur = torch.cuda.current_stream(self.torch_device)
        if (cur.cuda_stream or 0) == (self.stream() or 0):
            return False
        cur.synchronize()
        return True

    def _i32(a):
        """int32 vector of request indices; a value int32 cannot hold stays out of range"""
        return np.ascontiguousarray(np.clip(np.asarray(a, np.int64).reshape(-1), -1, 2 ** 31 - 1), np.int32)

    def crop_boxes(self, seg, mask_frame, mask_label, params: CropParams | None = None, device: bool = False):
        """mc_crop_boxes: (boxes int32 [n, levels, 4] = left, top, right, bottom; status int32 [n]) of the
        masks (mask_frame[i], mask_label[i]) in seg uint8 [F, H, W] (numpy, or a tensor on the context's
        device).  device=True: tensors on the context's device (no host wait when the context runs on
        torch's current stream); otherwise numpy arrays."""
        prm = params or crop_params()
        sp, sdev, F, H, W, _keep = _frames(self, seg, 0, "seg")
        mf, ml = _i32(mask_frame), _i32(mask_label)
        if len(mf) != len(ml):
            raise ValueError("mask_frame and mask_label differ in length")
        n, L = len(mf), int(prm.levels)
        if device:
            import torch
            boxes = torch.zeros((n, max(L, 0), 4), dtype=torch.int32, device=self.torch_device)
            status = torch.zeros(n, dtype=torch.int32, device=self.torch_device)
            settle = _order(self)
            bp, stp = ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(status.data_ptr())
        else:
            boxes, status = np.zeros((n, max(L, 0), 4), np.int32), np.zeros(n, np.int32)
            bp, stp = _ptr(boxes), _ptr(status)
            settle = False   # host outputs: the call waits itself
            if sdev:
                _order(self)
        self._check(self.L.mc_crop_boxes(self.h, F, H, W, sp, sdev, n, _ptr(mf), _ptr(ml), ctypes.byref(prm), bp, stp,
                                         1 if device else 0))
        if settle:
            self.synchronize()
        return boxes, status

    def crop_render(self, rgb, mask_frame, boxes, status, params: CropParams | None = None, out=None):
        """mc_crop_render: float32 [n, levels, 3, S, S] on the context's device for one chunk of masks.
        rgb uint8 [F, H, W, 3] (numpy or device tensor); boxes / status as crop_boxes returned them
        (numpy, or device tensors).  With the context on torch's current stream (set_stream) the call
        is stream-ordered and nothing waits; otherwise the host waits for the context's stream."""
        import torch
        prm = params or crop_params()
        rp, rdev, F, H, W, _keep = _frames(self, rgb, 3, "rgb")
        mf = _i32(mask_frame)
        n, L, S = len(mf), int(prm.levels), int(prm.out_size)
        on_dev = hasattr(boxes, "data_ptr")
        if on_dev != hasattr(status, "data_ptr"):
            raise ValueError("boxes and status must both be numpy arrays or both device tensors")
        if on_dev:
            if boxes.dtype != torch.int32 or status.dtype != torch.int32 or boxes.device.type != "cuda" or \
                    status.device.type != "cuda" or not boxes.is_contiguous() or not status.is_contiguous():
                raise ValueError("boxes / status: contiguous int32 device tensors")
            if boxes.numel() != n * L * 4 or status.numel() != n:
                raise ValueError("boxes / status do not match the masks")
            bp, stp = ctypes.c_void_p(boxes.data_ptr()), ctypes.c_void_p(status.data_ptr())
        else:
            boxes = np.ascontiguousarray(boxes, np.int32)
            status = np.ascontiguousarray(status, np.int32)
            if boxes.size != n * L * 4 or status.size != n:
                raise ValueError("boxes / status do not match the masks")
            bp, stp = _ptr(boxes), _ptr(status)
        if out is None:
            out = torch.empty((n, max(L, 0), 3, max(S, 0), max(S, 0)), dtype=torch.float32, device=self.torch_device)
        elif out.dtype != torch.float32 or out.device.type != "cuda" or not out.is_contiguous() or \
                out.numel() != n * L * 3 * S * S:
            raise ValueError("out: a contiguous float32 device tensor [n, levels, 3, S, S]")
        settle = _order(self)
        self._check(self.L.mc_crop_render(self.h, F, H, W, rp, rdev, n, _ptr(mf), bp, stp, 1 if on_dev else 0,
                                          ctypes.byref(prm), ctypes.c_void_p(out.data_ptr())))
        if settle:
            self.synchronize()
        return out

    def crop_coeffs(self, in_size, out_size):
        """mc_crop_coeffs: (ksize, bounds int32 [out_size, 2], kk int32 [out_size, ksize]) computed on the device."""
        k = ctypes.c_int32(0)
        self._check(self.L.mc_crop_coeffs(self.h, int(in_size), int(out_size), ctypes.byref(k), None, None))
        bounds = np.zeros((int(out_size), 2), np.int32)
        kk = np.zeros((int(out_size), k.value), np.int32)
        self._check(self.L.mc_crop_coeffs(self.h, int(in_size), int(out_size), ctypes.byref(k), _ptr(bounds), _ptr(kk)))
        return k.value, bounds, kk

    for f in (crop_boxes, crop_render, crop_coeffs):
        setattr(Context, f.__name__, f)


_crop_methods()


MC_PROJ_OK, MC_PROJ_BEHIND, MC_PROJ_OUTSIDE = 0, 1, 2


def _proj_methods():
    def _order(self):
        """as the crops: wait for torch's current stream when the context runs on another one"""
        import torch
        cur = torch.cuda.current_stream(self.torch_device)
        if (cur.cuda_stream or 0) == (self.stream() or 0):
            return False
        cur.synchronize()
        return True

    def _arrays(self, items, device):
        """{name: (array, dtype name, shape)} -> (pointers, keep-alive): numpy arrays made contiguous, or
        device tensors checked; None stays NULL"""
        ptrs, keep = {}, []
        for name, (a, dt, shape) in items.items():
            if a is None:
                ptrs[name] = None
                continue
            if device:
                import torch
                if not hasattr(a, "data_ptr") or a.device.type != "cuda" or a.dtype != getattr(torch, dt) or \
                        not a.is_contiguous() or (shape is not None and tuple(a.shape) != tuple(shape)):
                    raise ValueError(f"{name}: a contiguous {dt} device tensor of shape {shape}")
                ptrs[name] = ctypes.c_void_p(a.data_ptr()) if a.numel() else None
            else:
                if hasattr(a, "detach"):
                    a = a.detach().cpu().numpy()
                a = np.ascontiguousarray(a, dt)
                if shape is not None:
                    a = a.reshape(shape)
                ptrs[name] = _ptr(a)
            keep.append(a)
        return ptrs, keep

    def _outputs(self, shapes, device):
        if device:
            import torch
            out = {k: torch.full(sh, -1, dtype=torch.int32, device=self.torch_device) for k, sh in shapes.items()}
            return out, {k: ctypes.c_void_p(v.data_ptr()) for k, v in out.items()}
        out = {k: np.full(sh, -1, np.int32) for k, sh in shapes.items()}
        return out, {k: _ptr(v) for k, v in out.items()}

    def proj_boxes(self, points, obj_pt_off, obj_pts, intrinsics, world_to_cam, width, height, req_object, req_frame,
                   device: bool = False, num_points: int | None = None):
        """mc_proj_boxes: (boxes int32 [n, 4] = min px, min py, max px, max py; status int32 [n]; inside
        int32 [n]) of the requests (req_object[i], req_frame[i]).  points float64 [P, 3] or None (the
        num_points points of set_points), the objects' point lists in CSR form, intrinsics float64 [F, 4],
        world_to_cam float64 [F, 4, 4].  All numpy, or all tensors on the context's device; device=True:
        the outputs are device tensors, otherwise numpy arrays."""
        on_dev = hasattr(obj_pt_off, "data_ptr") and obj_pt_off.device.type == "cuda"
        F = int(intrinsics.shape[0])
        n = int(req_object.shape[0]) if hasattr(req_object, "shape") else len(req_object)
        if points is None and num_points is None:
            raise ValueError("proj_boxes: num_points is needed without points")
        P = int(num_points) if points is None else int(points.shape[0])
        if not on_dev:
            clip = lambda a: np.clip(np.asarray(a, np.int64).reshape(-1), -1, 2 ** 31 - 1)  # noqa: E731
            req_object, req_frame = clip(req_object), clip(req_frame)
        p, keep = _arrays(self, dict(points=(points, "float64", (P, 3)), off=(obj_pt_off, "int64", None),
                                     pts=(obj_pts, "int32", None), intr=(intrinsics, "float64", (F, 4)),
                                     w2c=(world_to_cam, "float64", (F, 4, 4)), robj=(req_object, "int32", (n,)),
                                     rframe=(req_frame, "int32", (n,))), on_dev)
        K = int(obj_pt_off.shape[0]) - 1
        out, op = _outputs(self, dict(boxes=(n, 4), status=(n,), inside=(n,)), device)
        settle = _order(self) if (on_dev or device) else False
        if not n:
            op = dict(boxes=None, status=None, inside=None)
        self._check(self.L.mc_proj_boxes(self.h, P, p["points"], K, p["off"], p["pts"], F,
                                         p["intr"], p["w2c"], int(width), int(height), n, p["robj"], p["rframe"],
                                         1 if on_dev else 0, op["boxes"], op["status"], op["inside"], 1 if device else 0))
        if settle and device:
            self.synchronize()
        return out["boxes"], out["status"], out["inside"]

    def proj_top_views(self, intrinsics, world_to_cam, width, height, top_k: int = 9, points=None, device: bool = False):
        """mc_proj_top_views on the last pp_run* result: dict of top_pos, top_frame, status, inside int32
        [num_final, top_k] and boxes int32 [num_final, top_k, 4], -1 where an object has fewer masks.
        intrinsics float64 [F, 4] and world_to_cam float64 [F, 4, 4] (and points float64 [P, 3], None:
        the points of set_points): all numpy, or all tensors on the context's device.  device=True:
        device tensors, and with the context on torch's current stream nothing waits."""
        on_dev = hasattr(intrinsics, "data_ptr") and intrinsics.device.type == "cuda"
        F = int(intrinsics.shape[0])
        p, keep = _arrays(self, dict(points=(points, "float64", None), intr=(intrinsics, "float64", (F, 4)),
                                     w2c=(world_to_cam, "float64", (F, 4, 4))), on_dev)
        k = int(top_k)
        nf = self.pp_export_sizes()[0]
        kk = k if 1 <= k <= 16 else 0    # an invalid top_k is the library's to refuse: no output is sized by it
        out, op = _outputs(self, dict(top_pos=(nf, kk), top_frame=(nf, kk), boxes=(nf, kk, 4), status=(nf, kk),
                                      inside=(nf, kk)), device)
        settle = _order(self) if (on_dev or device) else False
        self._check(self.L.mc_proj_top_views(self.h, p["points"], F, p["intr"], p["w2c"], int(width), int(height),
                                             1 if on_dev else 0, k, op["top_pos"], op["top_frame"], op["boxes"],
                                             op["status"], op["inside"], 1 if device else 0))
        if settle and device:
            self.synchronize()
        return out

    for f in (proj_boxes, proj_top_views):
        setattr(Context, f.__name__, f)


_proj_methods()


CLOUD_INFO = ["num_points", "stages", "max_stage_points", "max_voxel_population", "bytes_held"]


def _cloud_methods():
    def _on_device(*arrays):
        dev = [hasattr(a, "data_ptr") and a.device.type == "cuda" for a in arrays if a is not None]
        if any(dev) and not all(dev):
            raise ValueError("all arrays on the host, or all tensors on the context's device")
        return bool(dev) and all(dev)

    def _settle(self):
        """work queued on torch's current stream is waited for when the context runs on another one"""
        import torch
        cur = torch.cuda.current_stream(self.torch_device)
        if (cur.cuda_stream or 0) != (self.stream() or 0):
            cur.synchronize()

    def _arg(a, dt, shape, name, device):
        if device:
            import torch
            if a.dtype != getattr(torch, dt) or not a.is_contiguous() or tuple(a.shape) != tuple(shape):
                raise ValueError(f"{name}: a contiguous {dt} device tensor of shape {tuple(shape)}")
            return a, (ctypes.c_void_p(a.data_ptr()) if a.numel() else None)
        if hasattr(a, "detach"):
            a = a.detach().cpu().numpy()
        a = np.asarray(a)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(shape)} expected, got {tuple(a.shape)}")
        a = np.ascontiguousarray(a, dt)
        return a, (_ptr(a) if a.size else None)

    def cloud_fuse(self, depth, rgb, intrinsics, poses, params: CloudParams | None = None):
        """mc_cloud_fuse_frames: depth float32 [F, H, W], rgb uint8 [F, H, W, 3], intrinsics float64 [F, 4]
        = fx, fy, cx, cy, poses float64 [F, 4, 4]; all numpy, or all tensors on the context's device.
        The result stays on the device (cloud_get, scene_use_cloud); returns cloud_info()."""
        dev = _on_device(depth, rgb, intrinsics, poses)
        if len(depth.shape) != 3:
            raise ValueError("depth: [F, H, W]")
        F, H, W = (int(x) for x in depth.shape)
        if tuple(rgb.shape) != (F, H, W, 3):
            raise ValueError(f"rgb: shape {(F, H, W, 3)} expected, got {tuple(rgb.shape)} (a colour image of "
                             "another size than depth is not resized)")
        keep = [_arg(depth, "float32", (F, H, W), "depth", dev), _arg(rgb, "uint8", (F, H, W, 3), "rgb", dev),
                _arg(intrinsics, "float64", (F, 4), "intrinsics", dev), _arg(poses, "float64", (F, 4, 4), "poses", dev)]
        if params is None:
            params = CloudParams()
            self.L.mc_cloud_params_default(ctypes.byref(params))
        if dev:
            _settle(self)
        self._check(self.L.mc_cloud_fuse_frames(self.h, F, H, W, keep[0][1], keep[1][1], keep[2][1], keep[3][1],
                                                1 if dev else 0, ctypes.byref(params)))
        return self.cloud_info()

    def cloud_voxel_down(self, points, colors=None, voxel_size: float = 0.005):
        """mc_cloud_voxel_down: one voxel_down_sample of points float64 [n, 3] (colours float64 [n, 3] or
        None) by the device routine of cloud_fuse; returns cloud_info()."""
        dev = _on_device(points, colors)
        n = int(points.shape[0])
        p = _arg(points, "float64", (n, 3), "points", dev)
        c = _arg(colors, "float64", (n, 3), "colors", dev) if colors is not None else (None, None)
        if dev:
            _settle(self)
        self._check(self.L.mc_cloud_voxel_down(self.h, n, p[1], c[1], float(voxel_size), 1 if dev else 0))
        return self.cloud_info()

    def cloud_info(self):
        """mc_cloud_info: dict of CLOUD_INFO (result points, voxel_down_sample runs, the largest run's input
        points, the largest voxel population, bytes held)."""
        out = np.zeros(5, np.int64)
        self._check(self.L.mc_cloud_info(self.h, _ptr(out)))
        return dict(zip(CLOUD_INFO, (int(x) for x in out)))

    def cloud_get(self, device: bool = False, colors: bool = True):
        """mc_cloud_get: (points, colors) float64 [n, 3] of the result as numpy arrays, or with device=True
        as tensors on the context's device; colors=False (or a result without colours asked so): None."""
        n = self.cloud_info()["num_points"]
        if device:
            import torch
            _settle(self)
            pts = torch.empty((n, 3), dtype=torch.float64, device=self.torch_device)
            col = torch.empty((n, 3), dtype=torch.float64, device=self.torch_device) if colors else None
            pp = ctypes.c_void_p(pts.data_ptr()) if n else None
            cp = ctypes.c_void_p(col.data_ptr()) if (colors and n) else None
            if colors and not n:  # the state check of the colours still runs
                cp = ctypes.c_void_p(torch.empty(1, dtype=torch.float64, device=self.torch_device).data_ptr())
        else:
            pts = np.empty((n, 3), np.float64)
            col = np.empty((n, 3), np.float64) if colors else None
            pp, cp = _ptr(pts), _ptr(col)
        self._check(self.L.mc_cloud_get(self.h, pp, cp, 1 if device else 0))
        return pts, col

    def scene_use_cloud(self):
        """mc_scene_use_cloud: the result's points, rounded to float32, become the scene points."""
        self._check(self.L.mc_scene_use_cloud(self.h))

    for f in (cloud_fuse, cloud_voxel_down, cloud_info, cloud_get, scene_use_cloud):
        setattr(Context, f.__name__, f)


_cloud_methods()


def paint_params(**kw) -> PaintParams:
    """The reference's constants (score_threshold 0.5, min_pixels 400) with optional overrides."""
    p = PaintParams()
    load().mc_paint_params_default(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise TypeError(f"unknown paint parameter {k}")
        setattr(p, k, v)
    return p


def _paint_methods():
    def labels_paint(self, masks, scores, inst_off, params: PaintParams | None = None, device: bool = False, shape=None,
                     mask_dtype=None, labels_out=None):
        """mc_labels_paint: (labels, status [F], num_kept [F], label_instance [F, 255], instance_area [N]).
        masks [N, H, W] uint8 / bool / float32 and scores float32 [N]: both numpy arrays, or both tensors
        on the context's device, or both device pointers (ints; then shape=(H, W) and mask_dtype are
        required); inst_off: F + 1 offsets into N.  labels is a uint8 [F, H, W] tensor on the context's
        device (or labels_out, a device pointer or tensor, returned as given).  device=True: the four small
        outputs are int32 tensors on the device and, with device inputs, nothing waits when the context
        runs on torch's current stream; otherwise they are numpy arrays."""
        import torch
        prm = params or paint_params()
        off = np.ascontiguousarray(np.asarray(inst_off, np.int64).reshape(-1))
        if len(off) < 1:
            raise ValueError("inst_off: F + 1 offsets")
        F = len(off) - 1
        ntot = int(off[-1])
        keep = []
        if isinstance(masks, int) or isinstance(scores, int):
            if not (isinstance(masks, int) and isinstance(scores, int)) or shape is None or mask_dtype is None:
                raise ValueError("device pointers: both masks and scores, with shape=(H, W) and mask_dtype")
            H, W = (int(x) for x in shape)
            mp, sp, dev, mdt = ctypes.c_void_p(masks), ctypes.c_void_p(scores), 1, int(mask_dtype)
        else:
            masks, scores = (a if hasattr(a, "shape") else np.asarray(a) for a in (masks, scores))
            on = [hasattr(a, "data_ptr") and a.device.type == "cuda" for a in (masks, scores)]
            if on[0] != on[1]:
                raise ValueError("masks and scores: both on the host, or both on the context's device")
            dev = 1 if on[0] else 0
            if len(masks.shape) != 3 or int(masks.shape[0]) != ntot or int(scores.shape[0]) != ntot or len(scores.shape) != 1:
                raise ValueError(f"masks [N, H, W] and scores [N] with N = inst_off[-1] = {ntot}")
            H, W = int(masks.shape[1]), int(masks.shape[2])
            if dev:
                if masks.dtype == torch.bool:
                    masks = masks.view(torch.uint8)
                if masks.dtype not in (torch.uint8, torch.float32):
                    raise ValueError("masks: uint8, bool or float32")
                mdt = MC_PAINT_F32 if masks.dtype == torch.float32 else MC_PAINT_U8
                masks, scores = masks.contiguous(), scores.to(torch.float32).contiguous()
                mp = ctypes.c_void_p(masks.data_ptr()) if ntot else None
                sp = ctypes.c_void_p(scores.data_ptr()) if ntot else None
            else:
                masks, scores = (a.detach().numpy() if hasattr(a, "detach") else a for a in (masks, scores))
                masks = np.asarray(masks)
                if masks.dtype == np.bool_:
                    masks = masks.view(np.uint8)
                if masks.dtype not in (np.uint8, np.float32):
                    raise ValueError("masks: uint8, bool or float32")
                mdt = MC_PAINT_F32 if masks.dtype == np.float32 else MC_PAINT_U8
                masks, scores = np.ascontiguousarray(masks), np.ascontiguousarray(scores, np.float32)
                mp, sp = (_ptr(masks), _ptr(scores)) if ntot else (None, None)
            keep = [masks, scores]
        if labels_out is None:
            labels = torch.empty((F, max(H, 0), max(W, 0)), dtype=torch.uint8, device=self.torch_device)
            lp = ctypes.c_void_p(labels.data_ptr()) if labels.numel() else None
        else:
            labels = labels_out
            lp = ctypes.c_void_p(labels if isinstance(labels, int) else labels.data_ptr())
        if device:
            outs = [torch.empty(n, dtype=torch.int32, device=self.torch_device) for n in (F, F, F * MC_PAINT_MAX_IDS, ntot)]
            ptrs = [ctypes.c_void_p(o.data_ptr()) if o.numel() else None for o in outs]
        else:
            outs = [np.zeros(n, np.int32) for n in (F, F, F * MC_PAINT_MAX_IDS, ntot)]
            ptrs = [_ptr(o) if o.size else None for o in outs]
        cur = torch.cuda.current_stream(self.torch_device)
        other = (cur.cuda_stream or 0) != (self.stream() or 0)
        if other:
            cur.synchronize()  # the inputs and the fresh outputs live on torch's stream
        self._check(self.L.mc_labels_paint(self.h, F, H, W, _ptr(off), mdt, mp, sp, dev, ctypes.byref(prm), lp, *ptrs,
                                           1 if device else 0))
        if other:
            self.synchronize()
        del keep
        outs[2] = outs[2].reshape(F, MC_PAINT_MAX_IDS)
        return (labels, *outs)

    Context.labels_paint = labels_paint


_paint_methods()


def bits_unpack(words, ncols):
    """(R, W) little-endian uint64 bit rows -> (R, ncols) bool, unpacked by mc_bits_unpack's host
    threads (no GPU needed)."""
    words = np.ascontiguousarray(words, dtype="<u8")
    R = words.shape[0]
    out = np.empty((R, ncols), np.bool_)
    if R and ncols:
        rc = load().mc_bits_unpack(_ptr(words), R, words.shape[1], ncols, _ptr(out))
        if rc != 0:
            raise McError(rc, "mc_bits_unpack: bad sizes")
    return out
