// mc_crop_plan.hpp — the arithmetic of the CLIP crop preparation shared by the host and the device
// (semantics/get_open-voc_features.py:49-82 and Pillow's ImagingResample set-up for 8 bits per channel):
// the level boxes of a mask, the square a crop is pasted into, and one row of the bicubic
// coefficient table.  Everything is float64 / int32 exactly as in C; no product feeds an addition
// through a fused multiply-add (contraction is off for this file, and the library is built with
// -ffp-contract=off).  Compiles as plain C++ (scripts/crop_plan_check.cpp) and inside the kernels.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_CROP_HD __host__ __device__ inline
#else
#define MC_CROP_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mc {

constexpr int kCropOk = 0;      // status of a mask
constexpr int kCropAbsent = 1;  // no pixel of the label in its frame (the reference's np.min raises)
constexpr int kCropEmpty = 2;   // a single pixel: every level's crop is 0 x 0
constexpr int kCropPrecisionBits = 22;  // Pillow: 32 - 8 - 2

// mask2box_multi_level (:49-61): level box of the inclusive pixel bounds (left, top, right, bottom)
MC_CROP_HD void crop_level_box(int left, int top, int right, int bottom, int H, int W, int level, double expansion,
                               int32_t out[4])
{
    if (level == 0) {
        out[0] = left, out[1] = top, out[2] = right, out[3] = bottom;
        return;
    }
    const int dx = right - left, dy = bottom - top;
    const int x_exp = static_cast<int>(static_cast<double>(dx < 0 ? -dx : dx) * expansion) * level;
    const int y_exp = static_cast<int>(static_cast<double>(dy < 0 ? -dy : dy) * expansion) * level;
    out[0] = left - x_exp > 0 ? left - x_exp : 0;
    out[1] = top - y_exp > 0 ? top - y_exp : 0;
    out[2] = right + x_exp < W ? right + x_exp : W;
    out[3] = bottom + y_exp < H ? bottom + y_exp : H;
}

// pad_into_square (:75-82): the crop rgb[top:bottom, left:right] pasted at (ox, oy) into an s x s square
struct CropSquare {
    int w, h, s, ox, oy;
};

MC_CROP_HD CropSquare crop_square(const int32_t box[4])
{
    CropSquare q;
    q.w = box[2] - box[0];
    q.h = box[3] - box[1];
    q.s = q.w > q.h ? q.w : q.h;
    q.ox = (q.s - q.w) / 2;
    q.oy = (q.s - q.h) / 2;
    return q;
}

// the table's width for one (in_size, out_size): 2 * ceil(support) + 1
MC_CROP_HD int crop_ksize(int in_size, int out_size)
{
    const double scale = static_cast<double>(in_size) / static_cast<double>(out_size);
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    int c = static_cast<int>(support);
    if (static_cast<double>(c) < support) c++;
    return 2 * c + 1;
}

MC_CROP_HD double crop_bicubic(double t)
{
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
}

// row xx of the table: *xmin and the tap count (returned); k[j * stride] = tap j as a 22-bit
// fixed-point integer, for j < count (the caller leaves or zeroes the rest of the row)
MC_CROP_HD int crop_coeff_row(int in_size, int out_size, int xx, int32_t *xmin_out, int32_t *k, int64_t stride)
{
    const double scale = static_cast<double>(in_size) / static_cast<double>(out_size);
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    const double center = (static_cast<double>(xx) + 0.5) * scale;
    int xmin = static_cast<int>(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = static_cast<int>(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    double ww = 0.0;
    for (int x = 0; x < n; x++) ww += crop_bicubic((static_cast<double>(x + xmin) - center + 0.5) / fs);
    for (int x = 0; x < n; x++) {
        double w = crop_bicubic((static_cast<double>(x + xmin) - center + 0.5) / fs);  // the same value as summed
        if (ww != 0.0) w /= ww;
        const double f = w * static_cast<double>(1 << kCropPrecisionBits);
        k[x * stride] = w < 0 ? static_cast<int32_t>(f - 0.5) : static_cast<int32_t>(f + 0.5);
    }
    *xmin_out = xmin;
    return n;
}

// one output value of a pass: (2^21 + sum) >> 22 clipped to [0, 255]
MC_CROP_HD int crop_clip8(int acc)
{
    const int v = acc >> kCropPrecisionBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// the widest table a render of frames H x W can need (a square's side is at most max(H, W))
MC_CROP_HD int crop_max_ksize(int H, int W, int out_size) { return crop_ksize(H > W ? H : W, out_size); }

}  // namespace mc
