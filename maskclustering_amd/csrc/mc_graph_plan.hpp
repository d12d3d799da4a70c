// mc_graph_plan.hpp — graph build and clustering: the decisions the host takes around the kernels.
// Pure host arithmetic (no HIP include, plain C++17), used by mc_graph_host.inl, mc_cluster_host.inl
// and mc_shard_host.inl and checked on the CPU by tests/test_graph_plan_cpu.py
// (scripts/graph_plan_check.cpp).  The kernels' constants come in as arguments (each is defined
// beside its kernel: the S3 limits in mc_s3_kernels.inl; mc_kernels.inl's table says where).  The rules:
//  * Frame starts: the kept masks are in frame order; fs[c] is the first mask of a frame >= c.
//  * Shard row cut: the mask rows go to the ranks in contiguous blocks of about equal point counts;
//    rank k starts at the first row at which the cumulative points reach ceil(tot * k / W).
//    tests/oracle_shard_ctx.py restates the same cut for the CPU model of a sharded context.
//  * S3 work lists: a wave per mask for the bulk (small), a workgroup per mask for masks above the
//    small limit (big), and for every mask when the wave kernel's frame or counter limits do not
//    hold; each list largest first, ties in row order, so the long masks start early.
//  * S4 replicas: the histogram kernel keeps R lane-indexed LDS copies of the F + 1 counters at an
//    odd stride; R is the largest power of two up to 32 whose copies fit kHistReplicaBytes (1 when
//    even one does not).  hist_lds_bytes / thresholds_lds_bytes are the LDS the two S4 kernels ask for
//    (dynamic + static); the host refuses a frame count whose request exceeds the device's limit
//    per workgroup instead of launching (72 KiB and 130 KiB at 16384 frames).
//  * S6 mode: connect_threshold <= 0 links every pair with enough observers (dense_obs); torch
//    compares the rate in float32 (ctf); NaN passes no comparison, so it stays sparse with no edge.
//  * Components route: levels t >= 1 of scenes up to kFusedComponentsMaxN0 level-0 nodes label the
//    components in one workgroup (one launch); level 0 and larger scenes take five launches.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace mc {

inline std::vector<int32_t> frame_starts(const int32_t *col, int M, int F)
{
    std::vector<int32_t> fs(F + 1, 0);
    int g = 0;
    for (int c = 0; c <= F; c++) {
        while (g < M && col[g] < c) g++;
        fs[c] = g;
    }
    return fs;
}

inline int max_masks_per_frame(const std::vector<int32_t> &fs)
{
    int mx = 0;
    for (size_t c = 1; c < fs.size(); c++) mx = std::max(mx, fs[c] - fs[c - 1]);
    return mx;
}

struct RowCut {
    int r0, r1;
};

// rows [r0, r1) of `rank` of `world`; h_off: the M + 1 cumulative point counts of the rows
inline RowCut shard_row_cut(const int32_t *h_off, int M, int rank, int world)
{
    const int64_t tot = h_off[M];
    auto cut = [&](int k) {  // first row whose cumulative points reach k/W of the total
        if (k <= 0) return 0;
        if (k >= world) return M;
        const int64_t target = (tot * k + world - 1) / world;
        return static_cast<int>(std::lower_bound(h_off, h_off + M + 1, static_cast<int32_t>(target)) - h_off);
    };
    const int r0 = std::min(cut(rank), M);
    return {r0, std::max(r0, std::min(cut(rank + 1), M))};
}

// limits of the wave-per-mask S3 kernel (kS3wFrameWords64, kS3wCounters, kS3SmallPts)
struct S3Limits {
    int frame_words64, counters, small_pts;
};

inline bool s3_wave_ok(int F, int max_per_frame, const S3Limits &lim)
{
    return F <= 64 * lim.frame_words64 && max_per_frame < lim.counters;
}

// stable counting sort by size, descending (std::stable_sort of C3's 81k rows took ~4 ms of host
// time); sizes above kS3CountSortMax would make the table the larger cost
constexpr int kS3CountSortMax = 1 << 22;

inline void s3_by_size_desc(const int32_t *h_off, std::vector<int> &v)
{
    if (v.size() < 2) return;
    auto size = [&](int g) { return h_off[g + 1] - h_off[g]; };
    int mx = 0;
    for (int g : v) mx = std::max(mx, size(g));
    if (mx > kS3CountSortMax) {
        std::stable_sort(v.begin(), v.end(), [&](int x, int y) { return size(x) > size(y); });
        return;
    }
    std::vector<int> start(mx + 2, 0);
    for (int g : v) start[mx - size(g) + 1]++;
    for (int i = 1; i <= mx + 1; i++) start[i] += start[i - 1];
    std::vector<int> out(v.size());
    for (int g : v) out[start[mx - size(g)]++] = g;
    v.swap(out);
}

struct S3Lists {
    std::vector<int> small, big;
};

inline S3Lists s3_work_lists(const int32_t *h_off, RowCut rows, int F, int max_per_frame, const S3Limits &lim)
{
    const bool wave_ok = s3_wave_ok(F, max_per_frame, lim);
    S3Lists l;
    for (int g = rows.r0; g < rows.r1; g++)
        (wave_ok && h_off[g + 1] - h_off[g] <= lim.small_pts ? l.small : l.big).push_back(g);
    s3_by_size_desc(h_off, l.small);
    s3_by_size_desc(h_off, l.big);
    return l;
}

constexpr size_t kHistReplicaBytes = 40 * 1024;

inline int hist_stride(int F) { return (F + 1) | 1; }

inline int hist_replicas(int F)
{
    int R = 32;
    while (R > 1 && static_cast<size_t>(R) * hist_stride(F) * 4 > kHistReplicaBytes) R >>= 1;
    return R;
}

// k_s4_hist: the two staged tiles (tile_bytes) and the R replicas, all dynamic
inline size_t hist_lds_bytes(int F, size_t tile_bytes)
{
    return tile_bytes + static_cast<size_t>(hist_replicas(F)) * hist_stride(F) * 4;
}

// k_s4_thresholds: F + 1 cumulative counts (u64, dynamic) beside its static arrays
inline size_t thresholds_lds_dynamic(int F) { return (static_cast<size_t>(F) + 1) * 8; }

inline size_t thresholds_lds_bytes(int F, size_t static_bytes) { return thresholds_lds_dynamic(F) + static_bytes; }

struct S6Mode {
    bool dense_obs;
    float ctf;
};

inline S6Mode s6_mode(double connect_threshold)
{
    const bool dense = !(connect_threshold > 0.0);
    return {dense && !std::isnan(connect_threshold), static_cast<float>(connect_threshold)};
}

constexpr int kFusedComponentsMaxN0 = 32768;

inline bool s6_components_fused(int t, int N0) { return t > 0 && N0 <= kFusedComponentsMaxN0; }

}  // namespace mc
