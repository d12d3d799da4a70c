// mc_bp_qcell.hpp — S1 ball query: the cell arithmetic of a slot's box on the 2r scene grid.
// Plain C++17 without a HIP include, usable from host and device: k_grid_count builds the scene grid with
// scene_cell, k_bp_query_lds (mc_bp_query.inl) enumerates the cells of a mask's float32 AABB and
// numbers them with these functions, and scripts/bp_qcell_check.cpp checks them on the CPU
// (tests/test_bp_qcell_cpu.py).
//  * scene_cell(v, inv) is the biased cell coordinate of v on a grid of cell width 1 / inv, clamped to
//    [0, 2 kCellBias).  It is monotone in v (a float product by inv >= 0, floor, the int conversion and
//    the clamp are all monotone), so every point with lo < p < hi on an axis has
//    scene_cell(lo) <= scene_cell(p) <= scene_cell(hi): the cell range of a box holds the cell of every
//    point strictly inside it.
//  * QcBox is that range: origin and extent per axis.  qc_cells_capped counts its cells without
//    overflow (2^21 cells per axis: the product does not fit 64 bits), saturating at cap + 1.
//  * qc_local numbers the box's cells x-fastest, from the packed key (21 bits per axis, as pack3) a scene
//    record carries; qc_cell_of is its inverse on [0, cells): a bijection.  Cells adjacent in x are
//    adjacent in number, so a row of the per-point walk is one contiguous range of the cell-sorted crop.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define MC_QC_HD __host__ __device__ __forceinline__
#else
#define MC_QC_HD inline
#endif

namespace mc {

constexpr int kCellBias = 1 << 20;  // scene-grid cell coordinates in [-2^20, 2^20)

MC_QC_HD int scene_cell(float v, float inv)
{
    const int c = static_cast<int>(floorf(v * inv));
    const int a = c > -kCellBias ? c : -kCellBias;
    return (a < kCellBias - 1 ? a : kCellBias - 1) + kCellBias;
}

MC_QC_HD unsigned long long qc_key(int x, int y, int z)
{
    return (static_cast<unsigned long long>(x) << 42) | (static_cast<unsigned long long>(y) << 21) |
           static_cast<unsigned long long>(z);
}

struct QcBox {
    int o[3];  // first cell per axis (biased)
    int n[3];  // cells per axis (>= 1 for lo <= hi)
};

// the cells of the float32 box [lo, hi] (lo <= hi per axis)
MC_QC_HD QcBox qc_box(const float lo[3], const float hi[3], float inv)
{
    QcBox b;
    for (int a = 0; a < 3; a++) {
        b.o[a] = scene_cell(lo[a], inv);
        b.n[a] = scene_cell(hi[a], inv) - b.o[a] + 1;
    }
    return b;
}

// cells of the box, or cap + 1 if there are more than cap (cap >= 0)
MC_QC_HD long long qc_cells_capped(const QcBox &b, int cap)
{
    if (b.n[0] <= 0 || b.n[1] <= 0 || b.n[2] <= 0) return 0;
    if (b.n[0] > cap || b.n[1] > cap || b.n[2] > cap) return static_cast<long long>(cap) + 1;
    const long long xy = static_cast<long long>(b.n[0]) * b.n[1];
    if (xy > cap) return static_cast<long long>(cap) + 1;
    const long long c = xy * b.n[2];
    return c > cap ? static_cast<long long>(cap) + 1 : c;
}

// the number in [0, cells) of the box cell with packed key k (a cell of the box)
MC_QC_HD int qc_local(unsigned long long k, const QcBox &b)
{
    const int x = static_cast<int>(k >> 42), y = static_cast<int>((k >> 21) & 0x1FFFFFull),
              z = static_cast<int>(k & 0x1FFFFFull);
    return (x - b.o[0]) + b.n[0] * ((y - b.o[1]) + b.n[1] * (z - b.o[2]));
}

// the (biased) cell with number d in [0, cells)
MC_QC_HD void qc_cell_of(int d, const QcBox &b, int &x, int &y, int &z)
{
    x = b.o[0] + d % b.n[0];
    y = b.o[1] + (d / b.n[0]) % b.n[1];
    z = b.o[2] + d / (b.n[0] * b.n[1]);
}

}  // namespace mc
