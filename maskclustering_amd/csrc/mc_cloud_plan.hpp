// mc_cloud_plan.hpp — the decisions of the scene point cloud fusion (mc_cloud_*; tasmap/tasmap2mct_format.py:216-284)
// that the host takes between kernels, and the two rules the host and the kernels share: the voxel index of a
// coordinate and the comparator schedule of the per-voxel sort.  Pure functions: the flush schedule of
// (F, buffer_frames), the hash table's size, a stage's bytes against the budget, the accept / refuse decision of
// a stage.  Compiles as plain C++ (scripts/cloud_plan_check.cpp, tests/test_cloud_plan_cpu.py) and inside
// the kernels.  Contraction is off: every operation is rounded where it stands.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MC_CLOUD_HD __host__ __device__ inline
#else
#define MC_CLOUD_HD inline
#endif

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace mc {

constexpr int kCloudTilePx = 1024;          // frame pixels one workgroup counts and compacts (4 per thread)
constexpr int kCloudKeyBits = 21;           // bits of one axis in the packed voxel key (S1's packing)
constexpr int64_t kCloudMaxAxis = int64_t(1) << kCloudKeyBits;  // a stage's extent in voxels, per axis, stays below
constexpr int64_t kCloudMaxPoints = int64_t(1) << 31;           // a stage's points stay below
constexpr uint64_t kCloudEmptyKey = ~uint64_t(0);               // a free table entry (no packed key has bit 63)
constexpr int64_t kCloudSlack = 1 << 16;    // bytes of the small arrays of a stage (bounds, flags, scan partials)

// Population classes of the ordered fold.  A voxel of up to kCloudThreadMax points is sorted and folded by
// one thread (k_cloud_fold_small); one of up to kCloudLdsMax by a workgroup with its list in LDS
// (k_cloud_fold_block<true>); a larger one by a workgroup that sorts the list where it lies in global
// memory (k_cloud_fold_block<false>).
constexpr int kCloudThreadMax = 16;
constexpr int kCloudLdsMax = 4096;
constexpr int kCloudFoldChunk = 256;        // points the block fold stages per turn (one per thread)

// The reference's loop (:271-280): frame i joins the buffer, and the buffer is flushed when (i + 1) % B == 0;
// a non-empty remainder is flushed after the loop.  Stage k is frames [first, second).
inline std::vector<std::pair<int, int>> cloud_flush_schedule(int64_t F, int64_t B)
{
    std::vector<std::pair<int, int>> out;
    if (F <= 0 || B < 1) return out;
    int64_t start = 0;
    for (int64_t i = 0; i < F; i++)
        if ((i + 1) % B == 0) {
            out.emplace_back(static_cast<int>(start), static_cast<int>(i + 1));
            start = i + 1;
        }
    if (start < F) out.emplace_back(static_cast<int>(start), static_cast<int>(F));
    return out;
}

// entries of the open-addressing table for n points: a power of two, at least 2 per point, at least 64
MC_CLOUD_HD uint64_t cloud_table_size(int64_t n)
{
    uint64_t t = 64;
    while (t < 2 * static_cast<uint64_t>(n < 0 ? 0 : n)) t <<= 1;
    return t;
}

MC_CLOUD_HD int cloud_table_log2(uint64_t t)
{
    int l = 0;
    while ((uint64_t(1) << l) < t) l++;
    return l;
}

// Bytes one voxel_down_sample of n points holds at its peak, the input and the output included: the input
// (24 B a point, colour_bytes a point of colour: 0, 3 or 24), the table (key, count, first index: 16 B an
// entry), per point its table slot, first flag, voxel number and list entry (4 B each, the scans one more
// entry), per voxel (at most n) count, offset and cursor, and the means (24 B, and 24 B of colour).
MC_CLOUD_HD int64_t cloud_stage_bytes(int64_t n, int colour_bytes)
{
    const int64_t t = static_cast<int64_t>(cloud_table_size(n));
    return n * (24 + colour_bytes) + 16 * t + 16 * (n + 1) + 12 * (n + 1) + n * (24 + (colour_bytes ? 24 : 0)) + kCloudSlack;
}

// bytes of a buffer's frames on the device when they arrive from the host: depth float32, colour 3 bytes,
// and per tile its count and offset
MC_CLOUD_HD int64_t cloud_frame_bytes(int64_t frames, int64_t H, int64_t W)
{
    const int64_t px = frames * H * W;
    return px * 7 + 8 * ((px + kCloudTilePx - 1) / kCloudTilePx + 2);
}

// the budget of a call: the caller's (mc_ctx_set_memory_budget) or four fifths of the free device memory
MC_CLOUD_HD int64_t cloud_byte_budget(int64_t mem_budget, uint64_t free_bytes)
{
    if (mem_budget > 0) return mem_budget;
    return static_cast<int64_t>(free_bytes / 5 * 4);
}

// the voxel index of coordinate p on an axis whose grid starts at vmin (Open3D VoxelDownSample):
// a rounded subtraction, a rounded division, floor
MC_CLOUD_HD int64_t cloud_voxel_index(double p, double vmin, double voxel)
{
    const double t = (p - vmin) / voxel;
    return static_cast<int64_t>(floor(t));
}

MC_CLOUD_HD double cloud_vmin(double mn, double voxel) { return mn - voxel * 0.5; }

MC_CLOUD_HD uint64_t cloud_pack_key(int64_t ix, int64_t iy, int64_t iz)
{
    return (static_cast<uint64_t>(ix) << (2 * kCloudKeyBits)) | (static_cast<uint64_t>(iy) << kCloudKeyBits) |
           static_cast<uint64_t>(iz);
}

MC_CLOUD_HD uint64_t cloud_hash(uint64_t key, int log2_table)
{
    return (key * 0x9E3779B97F4A7C15ull) >> (64 - log2_table);
}

// What the host decides about a stage from its point count and bounds.  0: run it; otherwise the error
// code, with the message in *why.  (Codes as in mcgraph.h: 1 invalid, 5 unsupported.)
constexpr int kCloudAccept = 0, kCloudInvalid = 1, kCloudUnsupported = 5;

inline int cloud_check_count(int64_t n, int colour_bytes, int64_t extra_bytes, int64_t budget, std::string *why)
{
    if (n >= kCloudMaxPoints) {
        *why = "a stage of 2^31 points or more (" + std::to_string(n) + ")";
        return kCloudUnsupported;
    }
    const int64_t need = cloud_stage_bytes(n, colour_bytes) + extra_bytes;
    if (need > budget) {
        *why = "the stage of " + std::to_string(n) + " points needs " + std::to_string(need) + " bytes, the budget is " +
               std::to_string(budget);
        return kCloudUnsupported;
    }
    return kCloudAccept;
}

// the largest voxel index of each axis is the index of the axis' maximum (the index is monotone in p)
inline int cloud_check_extent(const double mn[3], const double mx[3], bool finite, double voxel, std::string *why)
{
    if (!finite) {
        *why = "a non-finite point";
        return kCloudInvalid;
    }
    for (int r = 0; r < 3; r++) {
        const double t = (mx[r] - cloud_vmin(mn[r], voxel)) / voxel;
        if (!(floor(t) < static_cast<double>(kCloudMaxAxis))) {
            *why = "a stage spans 2^21 voxels or more on axis " + std::to_string(r);
            return kCloudUnsupported;
        }
    }
    return kCloudAccept;
}

// The per-voxel sort is a bitonic network whose comparators all point upward, so that entries past the
// list's end act as +infinity without being stored: for k = 2, 4, ... (< 2 n) the first step pairs i with
// i ^ (k - 1) (the mirror inside its block of k), the steps j = k/4, k/8, ... 1 pair i with i ^ j.  A pair
// (i, l) is taken by its lower index i when l < n, and leaves the smaller value at i.
// cloud_sort_partner returns l for the lower index of a pair, -1 otherwise.
MC_CLOUD_HD int64_t cloud_sort_partner(int64_t i, int64_t k, int64_t j, int64_t n)
{
    const int64_t l = j == 0 ? (i ^ (k - 1)) : (i ^ j);
    return (l > i && l < n) ? l : -1;
}

}  // namespace mc
