// mc_paint_plan.hpp — the pure decisions and bit arithmetic of the label painter (mc_labels_paint; the
// reference's mask_predict.py:94-113), shared by the host driver and the kernels: the refusals with
// their messages, the rounds of frames that fit the scratch budget, the selection / order / id rule of
// one instance, and the three bit tricks of the kernels (four mask bytes -> four bits, the bit-sliced
// label fold, the 8 x 8 bit transpose).  Compiles as plain C++ (scripts/paint_plan_check.cpp) and
// inside the kernels.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_PAINT_HD __host__ __device__ inline
#else
#define MC_PAINT_HD inline
#endif

namespace mc {

constexpr int kPaintAccept = 0, kPaintInvalid = 1, kPaintUnsupported = 2;  // a check's verdict
constexpr int kPaintMaxInstances = 1024;  // per frame (MC_PAINT_MAX_INSTANCES)
constexpr int kPaintMaxIds = 255;         // ids of a uint8 image: the 256th kept instance overflows
constexpr int kPaintU8 = 0, kPaintF32 = 1;
constexpr int64_t kPaintDefaultBudget = 1ll << 30;  // scratch bytes of one round without a budget set
constexpr int kPaintLanePixels = 16;                // pixels a lane packs per step
constexpr int kPaintWavePixels = 64 * kPaintLanePixels;

MC_PAINT_HD int64_t paint_words(int64_t hw) { return (hw + 63) / 64; }  // 64-bit words of one bit plane
MC_PAINT_HD int paint_value_bytes(int mask_dtype) { return mask_dtype == kPaintF32 ? 4 : 1; }

// the arguments that are refused before anything is launched (message in *why)
inline int paint_check_args(int32_t num_frames, int32_t H, int32_t W, const int64_t *inst_off, int32_t mask_dtype,
                            int32_t min_pixels, std::string *why)
{
    auto no = [&](const char *m) {
        if (why) *why = m;
        return kPaintInvalid;
    };
    if (num_frames < 0) return no("negative number of frames");
    if (H <= 0 || W <= 0) return no("non-positive H or W");
    if (static_cast<int64_t>(H) * W > 2147483647ll) return no("H * W above 2^31 - 1");
    if (mask_dtype != kPaintU8 && mask_dtype != kPaintF32) return no("unknown mask_dtype");
    if (min_pixels < 0) return no("negative min_pixels");
    if (!inst_off) return no("null inst_off");
    if (inst_off[0] != 0) return no("inst_off[0] != 0");
    for (int f = 0; f < num_frames; f++) {
        if (inst_off[f + 1] < inst_off[f]) return no("inst_off not non-decreasing");
        if (inst_off[f + 1] - inst_off[f] > kPaintMaxInstances) {
            if (why) *why = "frame " + std::to_string(f) + ": more than MC_PAINT_MAX_INSTANCES (1024) instances";
            return kPaintInvalid;
        }
    }
    return kPaintAccept;
}

// scratch bytes of n instances in one round: their bit planes and, for host inputs, the staged masks
MC_PAINT_HD int64_t paint_round_bytes(int64_t n, int64_t hw, int mask_dtype, bool staged)
{
    return n * (paint_words(hw) * 8 + (staged ? hw * paint_value_bytes(mask_dtype) : 0));
}

inline int64_t paint_byte_budget(int64_t user_budget) { return user_budget > 0 ? user_budget : kPaintDefaultBudget; }

// consecutive frames [first, second) per round, as many as fit the budget; a frame that alone does not
// fit is refused.  Frames without instances join the round at hand.
inline int paint_rounds(int32_t num_frames, const int64_t *inst_off, int64_t hw, int mask_dtype, bool staged,
                        int64_t budget, std::vector<std::pair<int, int>> *rounds, std::string *why)
{
    rounds->clear();
    int f0 = 0;
    for (int f = 0; f < num_frames; f++) {
        const int64_t one = paint_round_bytes(inst_off[f + 1] - inst_off[f], hw, mask_dtype, staged);
        if (one > budget) {
            if (why)
                *why = "frame " + std::to_string(f) + " alone needs " + std::to_string(one) +
                       " bytes of scratch, above the memory budget of " + std::to_string(budget);
            rounds->clear();
            return kPaintUnsupported;
        }
        if (paint_round_bytes(inst_off[f + 1] - inst_off[f0], hw, mask_dtype, staged) > budget) {
            rounds->emplace_back(f0, f);
            f0 = f;
        }
    }
    if (f0 < num_frames) rounds->emplace_back(f0, num_frames);
    return kPaintAccept;
}

// rule 1: selected iff score >= threshold in float32 (a NaN score never is)
MC_PAINT_HD bool paint_selected(float score, float threshold) { return score >= threshold; }

// rule 2: instance j (score sj) is painted before instance i (score si): ascending score, ties (-0.0 and
// +0.0 included) by ascending index.  Only called on selected instances, so neither score is NaN.
MC_PAINT_HD bool paint_before(float sj, int j, float si, int i) { return sj < si || (sj == si && j < i); }

// bits 0..3 = (byte k of x == 1), exactly
MC_PAINT_HD uint32_t paint_bits4_u8(uint32_t x)
{
    const uint32_t y = x ^ 0x01010101u;                                         // a byte is 0 iff it was 1
    const uint32_t t = ~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu);  // 0x80 in every zero byte
    return (((t >> 7) * 0x00204081u) >> 21) & 0xfu;                             // bits 0, 8, 16, 24 -> 21..24
}

// the bits of `newly` take the id: plane b of the eight bit-sliced label planes holds bit b of each pixel's id
MC_PAINT_HD void paint_fold(uint64_t plane[8], uint64_t newly, int id)
{
    for (int b = 0; b < 8; b++)
        if ((id >> b) & 1) plane[b] |= newly;
}

// an 8 x 8 bit matrix (row r = byte r, column c = bit c) transposed
MC_PAINT_HD uint64_t paint_transpose8(uint64_t x)
{
    uint64_t t = (x ^ (x >> 7)) & 0x00aa00aa00aa00aaull;
    x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000cccc0000ccccull;
    x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000f0f0f0f0ull;
    x ^= t ^ (t << 28);
    return x;
}

// the eight label bytes of pixels 8g .. 8g + 7 of a word (byte p = pixel 8g + p, little-endian)
MC_PAINT_HD uint64_t paint_label_bytes(const uint64_t plane[8], int g)
{
    uint64_t rows = 0;
    for (int b = 0; b < 8; b++) rows |= ((plane[b] >> (8 * g)) & 0xffull) << (8 * b);
    return paint_transpose8(rows);
}

}  // namespace mc
