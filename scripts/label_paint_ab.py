"""Label images from instance masks at the C2 shape, in one process on one GPU:
  (device)   mc_labels_paint with the masks resident on the device, uint8 and float32;
  (loop)     the reference's loop (mask_predict.py:94-113) restated in torch on the device masks, with its
             per-mask ``.cpu().numpy()`` paints: what a predictor script runs today;
  (host)     the numpy restatement (tests/label_paint_restatement.py) on host copies of the masks.
Input: --frames frames of 480 x 640 with about --instances disc-shaped instances each (radii drawn so
that some fall below 400 pixels), scores uniform in [0, 1]; generated on the device from a seed.  The
two baselines walk the frames one by one, so they are run on the first --baseline-frames frames only and
reported per frame; all three results are compared bit for bit on those frames before anything is timed.
Device time: a host clock around the call and a synchronise, one warm-up, then --repeats runs (median,
min, max); the per-kernel timers of one further run; achieved bytes per second of the whole call against
the model  sum(N) * H * W * b * (1 + 1 / (8 b)) + F * H * W  (b = bytes per mask value: every value read
once, its bit written and read once, every label written once).  Prints one JSON line.
GPU run: python scripts/label_paint_ab.py [--frames 250] [--f32-frames 60] [--instances 100] [--repeats 7]"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import label_paint_restatement as R  # noqa: E402
from maskclustering_amd import _native  # noqa: E402

TIMERS = ("paint_pack", "paint_plan", "paint_image")
H, W = 480, 640


def make_frames(F, n_mean, seed):
    """(masks uint8 [N, H, W] on the device, scores float32 [N] on the device, inst_off)"""
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    counts = rng.integers(max(1, n_mean - 20), n_mean + 21, F)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    masks = torch.empty((int(off[-1]), H, W), dtype=torch.uint8, device="cuda")
    yy = torch.arange(H, device="cuda", dtype=torch.float32).view(1, H, 1)
    xx = torch.arange(W, device="cuda", dtype=torch.float32).view(1, 1, W)
    for f in range(F):
        n = int(counts[f])
        u = torch.rand((3, n), generator=g, device="cuda")
        cy, cx, r = (u[0] * H).view(n, 1, 1), (u[1] * W).view(n, 1, 1), (4 + u[2] * 120).view(n, 1, 1)
        masks[off[f]:off[f + 1]] = ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r).to(torch.uint8)
    scores = torch.rand(int(off[-1]), generator=g, device="cuda")
    return masks, scores, off


def reference_loop(pred_masks, pred_scores, threshold=0.5):
    """mask_predict.py:94-113 on one frame's device tensors, as written there"""
    import torch
    selected_indexes = (pred_scores >= threshold)
    selected_scores = pred_scores[selected_indexes]
    selected_masks = pred_masks[selected_indexes]
    _, m_H, m_W = selected_masks.shape
    mask_image = np.zeros((m_H, m_W), dtype=np.uint8)
    mask_id = 1
    selected_scores, ranks = torch.sort(selected_scores)
    for index in ranks:
        num_pixels = torch.sum(selected_masks[index])
        if num_pixels < 400:
            continue
        mask_image[(selected_masks[index] == 1).cpu().numpy()] = mask_id
        mask_id += 1
    return mask_image


def stats(ms, repeats):
    return dict(median=round(float(np.median(ms)), 3), min=round(min(ms), 3), max=round(max(ms), 3), repeats=repeats)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--f32-frames", type=int, default=60)
    ap.add_argument("--instances", type=int, default=100)
    ap.add_argument("--baseline-frames", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    masks, scores, off = make_frames(a.frames, a.instances, a.seed)
    ctx = _native.Context(0)
    prm = _native.paint_params()
    torch.cuda.synchronize()
    out = {"what": "label images from instance masks: mc_labels_paint vs the reference's loop on device masks vs numpy",
           "device": torch.cuda.get_device_name(0), "frames": [a.frames, H, W], "instances": int(off[-1])}

    # ---- the three routes agree on the baseline frames -------------------------------------------------
    B = min(a.baseline_frames, a.frames, a.f32_frames)
    nb = int(off[B])
    res = ctx.labels_paint(masks, scores, off, prm)
    got = res[0].cpu().numpy()
    assert not res[1].any(), "a frame overflowed"
    hm, hs = masks[:nb].cpu().numpy(), scores[:nb].cpu().numpy()
    t0 = time.perf_counter()
    want = R.paint_frames(hm, hs, off[:B + 1])
    host_ms = (time.perf_counter() - t0) * 1e3 / B
    loop = np.stack([reference_loop(masks[off[f]:off[f + 1]].float(), scores[off[f]:off[f + 1]]) for f in range(B)])
    out["bit_equal"] = bool(got[:B].tobytes() == want["labels"].tobytes() and loop.tobytes() == want["labels"].tobytes()
                            and res[2][:B].tobytes() == want["num_kept"].tobytes()
                            and res[4][:nb].tobytes() == want["instance_area"].tobytes())
    out["kept_per_frame_mean"] = round(float(res[2].mean()), 1)
    del hm, res

    # ---- the device routine -------------------------------------------------------------------------
    def timed(m, s, o):
        F, n = len(o) - 1, int(o[-1])
        b = m.element_size()
        ctx.labels_paint(m, s, o, prm, device=True)  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            ctx.labels_paint(m, s, o, prm, device=True)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ctx.set_timing(True)
        ctx.reset_kernel_times()
        ctx.labels_paint(m, s, o, prm, device=True)
        ctx.synchronize()
        kern = {k: round(ctx.kernel_time(k)[0], 3) for k in TIMERS}
        ctx.set_timing(False)
        model = n * H * W * b * (1 + 1 / (8 * b)) + F * H * W
        st = stats(ms, a.repeats)
        return dict(frames=F, instances=n, ms=st, ms_per_frame=round(st["median"] / F, 4), kernels_ms=kern,
                    model_bytes=int(model), call_GBps=round(model / st["median"] / 1e6, 1),
                    pack_GBps=round(n * H * W * (b + 1 / 8) / max(kern["paint_pack"], 1e-9) / 1e6, 1))

    out["device_uint8"] = timed(masks, scores, off)
    Ff = min(a.f32_frames, a.frames)
    mf = masks[:int(off[Ff])].float()
    out["device_float32"] = timed(mf, scores[:int(off[Ff])].contiguous(), off[:Ff + 1])

    # ---- a streaming kernel of the project on the same GPU, for scale: k_frames_decode ---------------------
    F = a.frames
    raw = torch.randint(0, 30000, (F, H, W), dtype=torch.int16, device="cuda")  # the bits of uint16 depths
    seg_in = torch.randint(0, 255, (F, H, W), dtype=torch.uint8, device="cuda")
    d_out = torch.empty((F, H, W), dtype=torch.float32, device="cuda")
    s_out = torch.empty((F, H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    decode = lambda: ctx.frames_decode(F, H, W, raw.data_ptr(), 1000.0, (H, W), seg_in.data_ptr(), True,  # noqa: E731
                                       d_out.data_ptr(), s_out.data_ptr())
    decode()
    ctx.set_timing(True)
    ctx.reset_kernel_times()
    for _ in range(a.repeats):
        decode()
    ms = ctx.kernel_time("frames_decode")[0] / a.repeats
    ctx.set_timing(False)
    out["frames_decode"] = dict(kernel_ms=round(ms, 3), GBps=round(F * H * W * 8 / ms / 1e6, 1))  # 2 + 1 in, 4 + 1 out
    del raw, seg_in, d_out, s_out

    # ---- the baselines, per frame -----------------------------------------------------------------------
    ms = []
    for f in range(B):  # the loop's float masks are the model's output: made before the clock starts
        pm, ps = mf[off[f]:off[f + 1]], scores[off[f]:off[f + 1]]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        reference_loop(pm, ps)
        ms.append((time.perf_counter() - t0) * 1e3)
    out["reference_loop_ms_per_frame"] = stats(ms, B)
    out["numpy_restatement_ms_per_frame"] = round(host_ms, 2)
    out["loop_over_device"] = round(out["reference_loop_ms_per_frame"]["median"] / out["device_float32"]["ms_per_frame"], 1)
    print(json.dumps(out), flush=True)
    assert out["bit_equal"], "the three routes differ"


if __name__ == "__main__":
    main()
