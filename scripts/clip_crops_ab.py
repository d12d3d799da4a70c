"""CLIP crop preparation of one scene's representative masks, two routes, in one process:
  (device) mc_crop_boxes once + mc_crop_render in chunks of 64 masks into one reused buffer, frames
           resident on the device, requests taken from the mc_pp_export arrays of mc_pp_run_clustered;
  (host)   the same crops as the reference prepares them (get_open-voc_features.py:44-99): np.where
           box, three crops, white square, Pillow bicubic resize, ToTensor / Normalize in numpy, one
           process (the reference spreads this over 16 DataLoader workers).
The parent commit has no device route, so the host route is the baseline.  The scene is a synthetic
C2-shaped one (synthetic_frames, 250 frames of 480 x 640) with random RGB frames; the model is not run.
Device time: events on the context's stream around boxes + all chunks, one warm-up, then --repeats
runs (median, min, max), and the per-kernel timers of one further run.  Host time: wall clock of
one pass over --host-masks masks (default: all), scaled to the scene when fewer.  A sample of the
crops is compared bit for bit between the routes.  Prints one JSON line.
GPU run: python scripts/clip_crops_ab.py [--shape c2] [--repeats 7] [--host-masks N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from maskclustering_amd import _native  # noqa: E402
from maskclustering_amd._native import PPParams  # noqa: E402
from maskclustering_amd.semantics import get_open_voc_features as gf  # noqa: E402
from maskclustering_amd.synthetic_frames import make_frames_shape  # noqa: E402

TIMERS = ("crop_boxes", "crop_coeffs", "crop_h", "crop_v")
CHUNK = 64


def host_crops(rgb, seg, req, lut, S=224):
    """the reference's __getitem__ for the requests, one process: float32 [n, 3, 3, S, S]"""
    from PIL import Image
    H, W = seg.shape[1:]
    out = np.zeros((len(req), 3, 3, S, S), np.float32)
    for i, (f, lab) in enumerate(req):
        pos = np.where(seg[f] == lab)
        top, bottom, left, right = np.min(pos[0]), np.max(pos[0]), np.min(pos[1]), np.max(pos[1])
        for lv in range(3):
            xe, ye = int(abs(right - left) * 0.1) * lv, int(abs(bottom - top) * 0.1) * lv
            box = (left, top, right, bottom) if lv == 0 else (max(0, left - xe), max(0, top - ye), min(W, right + xe),
                                                              min(H, bottom + ye))
            im = Image.fromarray(rgb[f][box[1]:box[3], box[0]:box[2]].copy())
            s = max(im.size)
            if s == 0:
                continue
            sq = Image.new("RGB", (s, s), (255, 255, 255))
            sq.paste(im, ((s - im.size[0]) // 2, (s - im.size[1]) // 2))
            a = np.asarray(sq.resize((S, S), Image.BICUBIC))
            for c in range(3):
                out[i, lv, c] = lut[c][a[..., c]]
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="c2")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--host-masks", type=int, default=0)
    a = ap.parse_args()
    from maskclustering_amd.sweep import SceneSweep
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev, dt)  # noqa: E731
        sw = SceneSweep(0, bench.shape_thresholds(a.shape)[1], stream=stream.cuda_stream)
        ctx = sw.ctx
        fr = make_frames_shape(a.shape, seed=0, device="cuda:0")   # rendered on the device, returned as numpy
        sw.run_scene(t(fr.scene_points, torch.float32), t(fr.depth, torch.float32), t(fr.seg, torch.uint8),
                     t(fr.intrinsics, torch.float64), t(fr.poses.reshape(-1, 16), torch.float64),
                     post_process=PPParams(0.1, 4, 0.5, 0.8))
        req = gf.crop_requests_from_export(sw.objects(device=True), sw.run.mask_col, sw.run.mask_label)
        F, H, W = fr.seg.shape
        rgb = np.random.default_rng(0).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
        rgb_d, seg_d = t(rgb, torch.uint8), t(fr.seg, torch.uint8)
        prm = _native.crop_params()
        n = len(req)
        mf, ml = req[:, 0], req[:, 1]
        buf = torch.empty((CHUNK, 3, 3, 224, 224), dtype=torch.float32, device=dev)
        sample = min(n, 48)
        keep = torch.empty((sample, 3, 3, 224, 224), dtype=torch.float32, device=dev)

        def device_route(keep_sample=False):
            boxes, status = ctx.crop_boxes(seg_d, mf, ml, prm, device=True)
            for i0 in range(0, n, CHUNK):
                i1 = min(n, i0 + CHUNK)
                ctx.crop_render(rgb_d, mf[i0:i1], boxes[i0:i1], status[i0:i1], prm, out=buf[:i1 - i0])
                if keep_sample and i0 == 0:
                    keep.copy_(buf[:sample])
            return status

        status = device_route(True)                    # warm-up: buffers sized
        stream.synchronize()
        ok = status.cpu().numpy() == _native.MC_CROP_OK
        ms = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            device_route()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        ctx.set_timing(True)
        ctx.reset_kernel_times()
        device_route()
        ctx.synchronize()
        kernels = {k: round(ctx.kernel_time(k)[0], 3) for k in TIMERS}
        ctx.set_timing(False)

        lut = np.stack([(np.arange(256, dtype=np.float32) / np.float32(255) - np.float32(prm.mean[c])) /
                        np.float32(prm.std[c]) for c in range(3)])
        hm = n if a.host_masks <= 0 else min(n, a.host_masks)
        idx = np.flatnonzero(ok)[:hm]
        t0 = time.perf_counter()
        host = host_crops(rgb, fr.seg, [(int(mf[i]), int(ml[i])) for i in idx], lut)
        host_s = time.perf_counter() - t0
        cmp_idx = [k for k, i in enumerate(idx) if i < sample]
        same = bool(np.array_equal(host[cmp_idx].view(np.uint32), keep.cpu().numpy()[idx[cmp_idx]].view(np.uint32)))
    out = {"what": f"CLIP crop preparation of one {a.shape} scene: device route vs the host route (one process)",
           "device": torch.cuda.get_device_name(0), "frames": [int(F), int(H), int(W)], "masks": int(n),
           "masks_ok": int(ok.sum()), "crops": int(n) * 3, "chunk": CHUNK,
           "device_ms": dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3),
                             repeats=a.repeats),
           "device_kernels_ms": kernels, "host_masks_timed": int(len(idx)), "host_s": round(host_s, 3),
           "host_s_per_scene": round(host_s * ok.sum() / max(len(idx), 1), 3),
           "host_over_device": round(host_s * ok.sum() / max(len(idx), 1) * 1e3 / float(np.median(ms)), 1),
           "sample_bit_equal": same, "sample_compared": len(cmp_idx)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
