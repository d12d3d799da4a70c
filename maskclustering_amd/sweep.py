"""Scene-parallel sweep over many scenes (BASELINE configs[4]: the 312-scene ScanNet val sweep), as the
reference's ``run.py:33-50`` runs it: one process per GPU, scene i on rank i mod N, each process
running ``main.py``'s path scene after scene, no collective on the data path.

Per scene (S1-S6 from frames resident in HBM): the scene's points (``mc_scene_set_points``, which
makes the next back-projection build the scene's ball-query grid), ``mc_backproject`` of every frame,
the masks as the graph input, ``mc_graph_build`` + ``mc_cluster_run``.

With ``begin_evaluation`` and ``run_scene(..., post_process=..., gt_ids=...)`` every scene's final objects
are also matched against its ground truth on the device (``mc_ev_add_scan_clustered``) and
``evaluation()`` gives the reference's AP table over the sweep (evaluation/evaluate.py:53-224).
With N ranks every rank holds the examples of its own scenes: ``evaluation(group)`` gathers the ranks'
accumulations as state buffers (``mc_ev_state_export``) onto one rank and merges them there
(``mc_ev_state_merge``); ``save_evaluation`` / ``load_evaluation`` checkpoint the same buffer."""
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


def gather_states(state, group, dst: int = 0):
    """The ranks' evaluation state buffers (``Context.ev_state``: uint8 numpy arrays, or uint8 tensors)
    on group rank dst: a list with one uint8 tensor per rank there, None elsewhere.

    Two collectives: an all-gather of the sizes, then a gather of uint8 tensors padded to the
    largest size (an all-gather where the backend has no gather).  Host tensors under gloo, device
    tensors under RCCL ("nccl"), decided as ``frame_shard.gather_masks`` does."""
    import torch
    import torch.distributed as dist
    from .frame_shard import _comm_device, _gather_supported
    t = state if hasattr(state, "data_ptr") else torch.from_numpy(np.ascontiguousarray(state, np.uint8))
    world, me = dist.get_world_size(group), dist.get_rank(group)
    dev = _comm_device(group, t.device)
    n = t.numel()
    sizes = torch.empty(world, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(sizes, torch.tensor([n], dtype=torch.int64, device=dev), group=group)
    sizes = [int(x) for x in sizes.cpu().tolist()]
    nmax = max(sizes)                                   # a multiple of 8, as every state's size
    buf = torch.zeros(nmax, dtype=torch.uint8, device=dev)
    buf[:n] = t.to(dev)
    if _gather_supported(group):
        parts = [torch.empty(nmax, dtype=torch.uint8, device=dev) for _ in range(world)] if me == dst else None
        dist.gather(buf, parts, dst=dist.get_global_rank(group, dst), group=group)
        if me != dst:
            return None
    else:
        allp = torch.empty(world * nmax, dtype=torch.uint8, device=dev)
        dist.all_gather_into_tensor(allp, buf, group=group)
        if me != dst:
            return None
        parts = list(allp.view(world, nmax))
    return [parts[r][:sizes[r]] for r in range(world)]


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
        self._ev_cfg = (np.asarray(class_ids, np.int32).copy(), self._ev_overlaps, int(min_region_size), bool(no_class))

    def _table(self, ap, stats) -> dict:
        out = {"ap": ap, "stats": stats}
        out.update(compute_averages(ap, self._ev_overlaps, self._ev_labels))
        return out

    def evaluation(self, group=None, dst: int = 0, broadcast: bool = False) -> dict | None:
        """The AP table over the scenes evaluated so far: ``ap`` [C, O], ``stats`` [C, O, 4] and the
        reference's averages (``compute_averages``: nanmean over the classes, the 0.25 overlap kept apart).

        group (a torch.distributed process group, one rank per sweep process): the table over the
        scenes of every rank.  Each rank exports its accumulation as a state buffer (``mc_ev_state_export``),
        the buffers are gathered on group rank dst (``gather_states``), which merges them into a scratch
        accumulation (``mc_ev_state_merge``) and returns its table; the other ranks return None, or
        with broadcast the same dict.  The ranks' own accumulations are not changed and keep growing;
        a rank without scenes contributes an empty state.  Collective: every rank of the group calls it."""
        if group is None:
            return self._table(*self.ctx.ev_ap())
        import torch
        import torch.distributed as dist
        from . import _native
        from .frame_shard import _comm_device
        dev = _comm_device(group, self.ctx.torch_device)
        me = dist.get_rank(group)
        states = gather_states(self.ctx.ev_state(device=dev.type == "cuda"), group, dst)
        C, O = len(self._ev_cfg[0]), len(self._ev_overlaps)
        res = torch.empty(C * O * 5, dtype=torch.int64, device=dev)      # ap's bits, then stats
        if me == dst:
            if getattr(self, "_ev_scratch", None) is None:
                self._ev_scratch = _native.Context(self.ctx.device_index)
            self._ev_scratch.ev_begin(*self._ev_cfg)
            for st in states:
                self._ev_scratch.ev_merge_state(st)
            ap, stats = self._ev_scratch.ev_ap()
            if not broadcast:
                return self._table(ap, stats)
            res.copy_(torch.from_numpy(np.concatenate([ap.view(np.int64).ravel(), stats.ravel()])))
        elif not broadcast:
            return None
        dist.broadcast(res, dist.get_global_rank(group, dst), group=group)
        res = res.cpu().numpy()
        return self._table(res[:C * O].view(np.float64).reshape(C, O).copy(), res[C * O:].reshape(C, O, 4).copy())

    def save_evaluation(self, path) -> None:
        """The accumulation so far to a file: its state buffer (include/mcgraph.h) and nothing else.
        With ``load_evaluation`` the checkpoint of a long sweep."""
        with open(path, "wb") as f:
            f.write(self.ctx.ev_state().tobytes())

    def load_evaluation(self, path) -> None:
        """Merge a file written by ``save_evaluation`` into the current accumulation (after
        ``begin_evaluation`` with the same configuration; anything else is an McError)."""
        self.ctx.ev_merge_state(np.fromfile(path, np.uint8))

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

    def top_views(self, intrinsics, poses, width, height, top_k: int = 9, device: bool = False) -> dict:
        """Which frames show each final object best, and where in them (the geometry of the reference's
        ``get_top_images.py``; ``Context.proj_top_views``), after ``run_scene(..., post_process=...)``.
        intrinsics [F,4] and poses [F,16] camera -> world as ``run_scene`` takes them (device tensors
        or numpy); width, height: the image size the boxes are clipped to (the reference takes it from
        the intrinsics object, not from the frames).  The poses are inverted with numpy on the host,
        as the reference inverts them.  Returns ``top_pos`` (positions into the object's mask list of
        ``objects()``), ``top_frame``, ``status``, ``inside`` [num_final, top_k] and ``boxes``
        [num_final, top_k, 4], -1 where an object has fewer masks: numpy, or device tensors."""
        from ._device import as_numpy
        k = np.ascontiguousarray(as_numpy(intrinsics), np.float64).reshape(-1, 4)
        w2c = np.linalg.inv(np.asarray(as_numpy(poses), np.float64).reshape(-1, 4, 4))
        return self.ctx.proj_top_views(k, w2c, width, height, top_k=top_k, device=device)

    def pred_masks(self, device: bool = False):
        """The [P, num_final] uint8 matrix of the reference's prediction npz."""
        return self.ctx.pp_pred_masks(self.run.P, device=device)
