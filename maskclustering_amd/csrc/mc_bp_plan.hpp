// mc_bp_plan.hpp — S1 batch planning: the frames a batch takes and the mask pixels its arrays hold.
// Pure host arithmetic (no HIP include, plain C++17), used by bp_run (mc_bp_host.inl) and checked on
// the CPU by tests/test_bp_plan_cpu.py (scripts/bp_plan_check.cpp).  The rules:
//  * HBM of the per-batch arrays (bp_reserve): kBpBytesPerMaskPixel per mask pixel (the arrays indexed
//    by pixel-list position, voxel and point arrays included), kBpBytesPerFramePixel per frame pixel
//    (the valid-id map); the per-slot and per-frame arrays are small against them.
//  * Byte budget: the context's own (mc_ctx_set_memory_budget), else 40 % of the device or 65 % of what
//    is free plus what the context already holds, whichever is less, so that a caller's allocator keeps
//    room (a fresh 288 GB device: ~115 GB); a caller that owns the device sets a larger one.
//  * Pixel budget: frame pixels per batch within the byte budget at the expected share of mask pixels
//    among frame pixels (1 before any batch, then the share seen; C3: 0.23, so two batches, not six:
//    the per-batch tails and syncs cost ~3 ms each, profiles/r05/r5s_*), at least a frame, below 2^31
//    (int positions).  Large batches amortise every group's slot tail and the per-batch sync (C3 E2E:
//    192 M pixels 215 ms, 600 M 175 ms in round 2; 1 G 115 ms against 118 ms at 640 M in round 3,
//    profiles/r03/ab19_batch_pixels.jsonl).
//  * Frames per batch: the pixel budget in whole frames, then dealt into equal batches (no small
//    remainder batch with its own tails).  Frames staged from the host upload batch b + 1 under batch
//    b's compute; splitting a scene that fits one batch only for that did not pay (C2 API path: 1 batch
//    44.9 ms, 8 batches 46.2 ms, profiles/r03/api/), so only MC_BP_UPLOAD_BATCHES=n forces n batches.
//  * Mask-pixel capacity: the batch's frame pixels times the expected share, plus 1/16 and a frame's
//    worth, never more than every pixel of the batch.
//  * A batch with more mask pixels than the capacity is redone at the share it showed: with fewer
//    frames if the byte budget asks for it (a denser scene than the share learned so far), else with
//    room for every pixel it listed.  Another overflow shrinks or grows again, so the redo terminates.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace mc {

constexpr size_t kBpBytesPerMaskPixel = 196;
constexpr size_t kBpBytesPerFramePixel = 2;

// bytes the per-batch arrays of these capacities hold
inline size_t bp_held_bytes(size_t mask_px_cap, size_t frame_px_cap)
{
    return mask_px_cap * kBpBytesPerMaskPixel + frame_px_cap * kBpBytesPerFramePixel;
}

// byte budget of the per-batch arrays; total_b == 0: the device's memory is unknown
inline size_t bp_byte_budget(int64_t mem_budget, size_t free_b, size_t total_b, size_t held)
{
    if (mem_budget > 0) return static_cast<size_t>(mem_budget);
    if (!total_b) return held;
    return std::min(total_b / 100 * 40, (free_b + held) / 100 * 65);
}

// frame pixels per batch within `bytes` at mask-pixel share mfrac
inline size_t bp_pixel_budget(size_t bytes, double mfrac, size_t HW)
{
    const size_t budget = (static_cast<size_t>(1) << 31) - 1;
    const double per_px = static_cast<double>(kBpBytesPerFramePixel) + mfrac * kBpBytesPerMaskPixel;
    return std::max<size_t>(HW, std::min(budget, static_cast<size_t>(static_cast<double>(bytes) / per_px)));
}

// frames per batch; upload_batches > 0: the frames are staged from the host in at least that many batches
inline int bp_frames_per_batch(int F, size_t HW, size_t budget, int upload_batches)
{
    int FB = static_cast<int>(std::max<size_t>(1, std::min<size_t>(std::max(F, 1), budget / HW)));
    const int nb = (std::max(F, 1) + FB - 1) / FB;
    FB = (std::max(F, 1) + nb - 1) / nb;
    if (upload_batches > 0) FB = std::max(1, std::min(FB, (F + upload_batches - 1) / upload_batches));
    return FB;
}

inline size_t bp_mask_cap(int FB, size_t HW, double frac)
{
    const double fpx = static_cast<double>(FB) * static_cast<double>(HW);
    return static_cast<size_t>(std::min(fpx, frac * fpx * 1.0625 + static_cast<double>(HW))) + 1024;
}

// frames per batch after a batch of FB frames overflowed at share frac
inline int bp_shrink_after_overflow(int FB, size_t HW, double frac, size_t bud_bytes, bool fixed_batch)
{
    if (fixed_batch) return FB;
    const double per_px = static_cast<double>(kBpBytesPerFramePixel) +
                          std::min(1.0, frac * 1.0625 + 1.0 / FB) * kBpBytesPerMaskPixel;
    const double fit = std::floor(static_cast<double>(bud_bytes) / (per_px * static_cast<double>(HW)));
    return std::max(1, std::min(FB, static_cast<int>(std::min(fit, 1e9))));
}

// mask-pixel capacity for the redo: fewer frames take the share's room, the same frames again room
// for every one of the npx pixels they listed
inline size_t bp_redo_mask_cap(int FB, int fb_was, size_t HW, double frac, size_t npx)
{
    return FB < fb_was ? bp_mask_cap(FB, HW, frac) : std::max(bp_mask_cap(FB, HW, frac), npx + 1024);
}

}  // namespace mc
