"""Scene-parallel sweep over many scenes (BASELINE configs[4]: the 312-scene ScanNet val sweep), as the
reference's ``run.py:33-50`` runs it: one process per GPU, scene i on rank i mod N, each process
running ``main.py``'s path scene after scene, no collective on the data path.

Per scene (S1-S6 from frames resident in HBM): the scene's points (``mc_scene_set_points``, which
makes the next back-projection build the scene's ball-query grid), ``mc_backproject`` of every frame,
the masks as the graph input, ``mc_graph_build`` + ``mc_cluster_run``.

With ``begin_evaluation`` and ``run_scene(..., post_process=..., gt_ids=...)`` every scene's final objects
are also matched against its ground truth on the device (``mc_ev_add_scan_clustered``) and
``evaluation()`` gives the reference's AP table over the sweep (evaluation/evaluate.py:53-224)."""
from __future__ import annotations

import warnings

import numpy as np


def scenes_of(rank: int, world: int, num_scenes: int) -> list[int]:
    """The scene numbers rank runs: i with i mod world == rank (run.py:33-50 hands scene lists to
    one process per GPU)."""
    if world < 1 or not 0 <= rank < world:
        raise ValueError(f"bad rank {rank} of {world}")
    return list(range(rank, int(num_scenes), world))


def compute_averages(ap, overlaps, class_labels) -> dict:
    """evaluation/evaluate.py:207-224 on a [C, O] table: ``all_ap`` (every overlap but 0.25),
    ``all_ap_50%``, ``all_ap_25%`` as nanmeans over the classes, and per class the plain averages."""
    ap, overlaps = np.asarray(ap), np.asarray(overlaps)
    o50, o25 = np.isclose(overlaps, 0.5), np.isclose(overlaps, 0.25)
    rest = np.logical_not(o25)
    with warnings.catch_warnings():               # a class without ground truth anywhere: nanmean of an empty slice
        warnings.simplefilter("ignore", RuntimeWarning)
        out = {"all_ap": np.nanmean(ap[:, rest]), "all_ap_50%": np.nanmean(ap[:, o50]),
               "all_ap_25%": np.nanmean(ap[:, o25]), "classes": {}}
    for li, name in enumerate(class_labels):
        out["classes"][name] = {"ap": np.average(ap[li, rest]), "ap50%": np.average(ap[li, o50]),
                                "ap25%": np.average(ap[li, o25])}
    return out


class SceneSweep:
    """One process's scenes on one device: ``run_scene`` per scene, the context reused across scenes
    (its S1 batches sized from the scenes before, within its HBM budget)."""

    def __init__(self, device: int, thresholds: dict, params=None, stream=None):
        from . import _native
        from .pipeline import GraphRun
        self.run = GraphRun(device)
        self.ctx = self.run.ctx
        if stream is not None:
            self.ctx.set_stream(stream)
        self.cfg = dict(thresholds)
        self.prm = params if params is not None else _native.bp_params()

    def begin_evaluation(self, class_ids, no_class=True, overlaps=None, min_region_size=100, class_labels=None):
        """Start (or reset) the AP accumulation of this sweep: the class table, the reference's
        ``--no_class`` switch, its overlaps (evaluate.py:44 by default) and minimum region size.
        class_labels name the classes in ``evaluation()`` (default: the ids as strings)."""
        self.ctx.ev_begin(class_ids, overlaps, min_region_size, no_class)
        self._ev_overlaps = np.append(np.arange(0.5, 0.95, 0.05), 0.25) if overlaps is None else np.asarray(overlaps, np.float64)
        self._ev_labels = [str(c) for c in class_ids] if class_labels is None else list(class_labels)
        if len(self._ev_labels) != len(class_ids):
            raise ValueError("class_labels and class_ids differ in length")

    def evaluation(self) -> dict:
        """The AP table over the scenes evaluated so far: ``ap`` [C, O], ``stats`` [C, O, 4] and the
        reference's averages (``compute_averages``: nanmean over the classes, the 0.25 overlap kept apart)."""
        ap, stats = self.ctx.ev_ap()
        out = {"ap": ap, "stats": stats}
        out.update(compute_averages(ap, self._ev_overlaps, self._ev_labels))
        return out

    def run_scene(self, points, depth, seg, intrinsics, poses, post_process=None, gt_ids=None) -> int:
        """points float32 [P,3], depth f32 [F,H,W], seg u8 [F,H,W], intrinsics f64 [F,4], poses f64
        [F,16]: contiguous torch tensors on the device.  Returns the scene's object count; the
        context holds the scene's full result (GraphRun.canonical, the getters).

        post_process: a ``PPParams``: the clustered objects are post-processed on the device as well
        (``mc_pp_run_clustered`` on the scene's float32 points) and the count of final objects is
        returned; ``objects()`` and ``pred_masks()`` give the reference's final product.

        gt_ids (with post_process, after ``begin_evaluation``): the scene's ground-truth ids [P]
        (int32 tensor on the device, or numpy); the scene is added to the evaluation."""
        if gt_ids is not None and post_process is None:
            raise ValueError("gt_ids needs post_process")
        for t in (points, depth, seg, intrinsics, poses):
            if t.device.type != "cuda" or not t.is_contiguous():
                raise ValueError("scene inputs must be contiguous device tensors")
        F, H, W = depth.shape
        self.ctx.set_points(device_ptr=points.data_ptr(), num_points=len(points))
        self.ctx.backproject(None, None, None, None, self.prm, shape=(F, H, W),
                             device_ptrs=(depth.data_ptr(), seg.data_ptr(), intrinsics.data_ptr(), poses.data_ptr()))
        col, lab, _ = self.ctx.bp_mask_index()
        self.run.P, self.run.F = len(points), F
        self.run.mask_col, self.run.mask_label = np.asarray(col), np.asarray(lab)
        self.ctx.use_backprojection()
        self.run.step(**self.cfg)
        if post_process is None:
            return int(self.ctx.cluster_info().num_objects)
        self.ctx.pp_run_clustered(post_process)
        if gt_ids is not None:
            self.ctx.ev_add_scan_clustered(gt_ids)
        return int(self.ctx.pp_info().num_final)

    def objects(self, device: bool = False) -> dict:
        """The final objects of the last ``run_scene(..., post_process=...)`` (``Context.pp_export``):
        per-object point lists, mask lists (rows of the scene's mask table: ``run.mask_col`` /
        ``run.mask_label``) with coverages, representative masks and source nodes."""
        return self.ctx.pp_export(device=device)

    def pred_masks(self, device: bool = False):
        """The [P, num_final] uint8 matrix of the reference's prediction npz."""
        return self.ctx.pp_pred_masks(self.run.P, device=device)
