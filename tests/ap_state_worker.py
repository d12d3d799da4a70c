"""Worker processes of the evaluation-state tests (tests/test_gpu_ap_state.py).

    python tests/ap_state_worker.py <mode> <backend> <rank> <world> <port> <out.npz>

All ranks share cuda:0.  Every rank builds a SceneSweep, adds its share of the work (item s with
s mod world == rank, sweep.scenes_of), calls ``evaluation(group, dst=0)`` and then
``evaluation(group, dst=0, broadcast=True)``, checks that its own accumulation's state is the same
bytes before and after, and saves what the two calls returned.
mode "golden:<ca|nc>:<nscans>": the first nscans scans of tests/golden/ap_small.npz through ev_add_scan.
mode "sweep": the three synthetic scenes of tests/test_gpu_ap.py::test_sweep_evaluation through run_scene.
backend "gloo" (host tensors) or "nccl" (device tensors)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import test_gpu_ap as T  # noqa: E402
from maskclustering_amd.sweep import scenes_of  # noqa: E402


def main():
    mode, backend, rank, world, port, out = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], sys.argv[6]
    torch.cuda.set_device(0)
    kw = dict(device_id=torch.device("cuda", 0)) if backend == "nccl" else {}
    dist.init_process_group(backend, init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, **kw)
    try:
        sw = T._sweep()
        if mode.startswith("golden:"):
            _, m, nscans = mode.split(":")
            z = T.golden()
            sw.begin_evaluation(z["class_ids"], no_class=m == "nc", overlaps=z["overlaps"],
                                min_region_size=int(z["min_region_size"]))
            for s in scenes_of(rank, world, int(nscans)):
                sw.ctx.ev_add_scan(z[f"s{s}_gt"], z[f"s{s}_off"], z[f"s{s}_pts"], z[f"s{s}_classes"], z[f"s{s}_scores"])
        else:
            from maskclustering_amd.synthetic_frames import make_frames_shape, slab_ground_truth
            sw.begin_evaluation(T.CLS, no_class=True)
            for s in scenes_of(rank, world, len(T.SCENES)):
                fr = make_frames_shape(T.SCENES[s][0], seed=T.SCENES[s][1])
                T._run(sw, fr, slab_ground_truth(fr.scene_points, T.CLS))
        own = sw.ctx.ev_state()
        res = {"own_state": own}
        for name, bc in (("dst", False), ("bc", True)):
            ev = sw.evaluation(dist.group.WORLD, dst=0, broadcast=bc)
            res[name + "_none"] = np.array(ev is None)
            if ev is not None:
                res[name + "_ap"], res[name + "_stats"] = ev["ap"], ev["stats"]
                res[name + "_avg"] = np.array([ev["all_ap"], ev["all_ap_50%"], ev["all_ap_25%"]])
            np.testing.assert_array_equal(sw.ctx.ev_state(), own)
        own_ap, own_stats = sw.ctx.ev_ap()
        res["own_ap"], res["own_stats"] = own_ap, own_stats
        np.savez(out, **res)
        dist.barrier()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
