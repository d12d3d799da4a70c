// Graph and clustering host decisions (maskclustering_amd/csrc/mc_graph_plan.hpp) on the CPU: worked
// cases of every function, the structural properties of the shard row cut on random offset tables, and
// the S3 work lists against std::stable_sort.  Built and run by tests/test_graph_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/graph_plan_check.cpp -o graph_plan_check && ./graph_plan_check
#include <cstdio>
#include <random>

#include "mc_graph_plan.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            printf("line %d: %s\n", __LINE__, #cond);                \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;
using vec32 = std::vector<int32_t>;

static vec32 offsets(const vec32 &sizes)
{
    vec32 off(sizes.size() + 1, 0);
    for (size_t i = 0; i < sizes.size(); i++) off[i + 1] = off[i] + sizes[i];
    return off;
}

static void frame_start_cases()
{
    CHECK((frame_starts(nullptr, 0, 0) == vec32{0}));           // F = 0
    CHECK((frame_starts(nullptr, 0, 3) == vec32{0, 0, 0, 0}));  // frames without a mask
    const vec32 col{2, 2, 3, 6, 6, 6};  // frames 0, 1 (leading), 4, 5 (middle), 7, 8 (trailing) empty
    CHECK((frame_starts(col.data(), 6, 9) == vec32{0, 0, 0, 2, 3, 3, 3, 6, 6, 6}));
    CHECK(max_masks_per_frame(frame_starts(col.data(), 6, 9)) == 3);
    const vec32 one{1, 1, 1, 1};  // all masks in one frame
    CHECK((frame_starts(one.data(), 4, 3) == vec32{0, 0, 4, 4}));
    CHECK(max_masks_per_frame(frame_starts(one.data(), 4, 3)) == 4);
    CHECK(max_masks_per_frame(frame_starts(nullptr, 0, 0)) == 0);
}

static bool cut_is(const vec32 &sizes, int W, const std::vector<RowCut> &want)
{
    const vec32 off = offsets(sizes);
    for (int r = 0; r < W; r++) {
        const RowCut c = shard_row_cut(off.data(), static_cast<int>(sizes.size()), r, W);
        if (c.r0 != want[r].r0 || c.r1 != want[r].r1) return false;
    }
    return true;
}

static void row_cut_cases()
{
    // results of the restatement in tests/oracle_shard_ctx.py (ShardCtx.build's cut), computed once
    CHECK(cut_is({5, 0, 3, 7, 0, 0, 2, 9, 1, 4}, 3, {{0, 4}, {4, 8}, {8, 10}}));
    CHECK(cut_is({10, 1, 1, 1, 1, 1, 1}, 4, {{0, 1}, {1, 1}, {1, 3}, {3, 7}}));  // a row above two shares
    CHECK(cut_is({0, 0, 4, 0}, 2, {{0, 3}, {3, 4}}));
    CHECK(cut_is({0, 0, 4, 0}, 5, {{0, 3}, {3, 3}, {3, 3}, {3, 3}, {3, 4}}));  // world > M
    CHECK(cut_is({1000000, 3, 2000000, 5}, 3, {{0, 2}, {2, 3}, {3, 4}}));
    CHECK(cut_is({2, 2, 2, 2, 2, 2}, 4, {{0, 2}, {2, 3}, {3, 5}, {5, 6}}));
    CHECK(cut_is({0, 0, 0}, 2, {{0, 0}, {0, 3}}));  // no points at all

    std::mt19937 rng(20241020);
    int broken = 0, unbalanced = 0, empty_blocks = 0;
    for (int it = 0; it < 3000; it++) {
        const int M = it % 50 == 0 ? 0 : static_cast<int>(rng() % 60);
        const int W = it % 7 == 0 ? 1 : 1 + static_cast<int>(rng() % (it % 3 ? 8 : 90));  // world > M too
        vec32 sizes(M);
        for (int &v : sizes) v = rng() % 3 == 0 ? 0 : static_cast<int>(rng() % (it % 5 ? 40 : 100000));
        const vec32 off = offsets(sizes);
        const int64_t tot = off[M], share = (tot + W - 1) / W;
        const int mx = M ? *std::max_element(sizes.begin(), sizes.end()) : 0;
        int next = 0;
        for (int r = 0; r < W; r++) {  // contiguous, disjoint, covering [0, M)
            const RowCut c = shard_row_cut(off.data(), M, r, W);
            broken += c.r0 != next || c.r1 < c.r0 || c.r1 > M;
            unbalanced += off[c.r1] - off[c.r0] > share + mx;
            empty_blocks += c.r0 == c.r1;
            next = c.r1;
        }
        broken += next != M;
    }
    CHECK(broken == 0);
    CHECK(unbalanced == 0);
    CHECK(empty_blocks > 100);  // the cases do hold ranks without rows
}

static std::vector<int> sorted_desc(const vec32 &off, std::vector<int> v)
{
    std::stable_sort(v.begin(), v.end(), [&](int x, int y) { return off[x + 1] - off[x] > off[y + 1] - off[y]; });
    return v;
}

// the two lists of rows [r0, r1) against a plain split and std::stable_sort
static int lists_differ(const vec32 &off, RowCut rows, int F, int mpf, const S3Limits &lim)
{
    const S3Lists l = s3_work_lists(off.data(), rows, F, mpf, lim);
    std::vector<int> small, big;
    for (int g = rows.r0; g < rows.r1; g++)
        (s3_wave_ok(F, mpf, lim) && off[g + 1] - off[g] <= lim.small_pts ? small : big).push_back(g);
    return (l.small != sorted_desc(off, small)) + (l.big != sorted_desc(off, big)) +
           (l.small.size() + l.big.size() != static_cast<size_t>(rows.r1 - rows.r0));
}

static void work_list_cases()
{
    const S3Limits lim{4, 32, 1024};  // up to 256 frames, fewer than 32 masks in a frame, 1024 points
    CHECK(s3_wave_ok(256, 31, lim) && !s3_wave_ok(257, 31, lim) && !s3_wave_ok(256, 32, lim));
    {  // ties keep the row order; a size equal to the limit is small
        const vec32 off = offsets({7, 1024, 1025, 7, 0, 3000, 1025, 7});
        const S3Lists l = s3_work_lists(off.data(), {0, 8}, 10, 3, lim);
        CHECK((l.small == std::vector<int>{1, 0, 3, 7, 4}));
        CHECK((l.big == std::vector<int>{5, 2, 6}));
        const S3Lists part = s3_work_lists(off.data(), {2, 6}, 10, 3, lim);  // a rank's rows only
        CHECK((part.small == std::vector<int>{3, 4}) && (part.big == std::vector<int>{5, 2}));
        const S3Lists all_big = s3_work_lists(off.data(), {0, 8}, 257, 3, lim);  // the predicate fails
        CHECK(all_big.small.empty() && (all_big.big == std::vector<int>{5, 2, 6, 1, 0, 3, 7, 4}));
        const S3Lists none = s3_work_lists(off.data(), {3, 3}, 10, 3, lim);
        CHECK(none.small.empty() && none.big.empty());
    }
    std::mt19937 rng(7);
    int differ = 0, nsmall = 0, nbig = 0;
    for (int it = 0; it < 1500; it++) {
        const int M = static_cast<int>(rng() % 80);
        vec32 sizes(M);
        for (int &v : sizes) v = static_cast<int>(rng() % (rng() % 4 ? 12 : 3000));  // many ties, some big
        const vec32 off = offsets(sizes);
        const int W = 1 + static_cast<int>(rng() % 4);
        const RowCut rows = shard_row_cut(off.data(), M, static_cast<int>(rng() % W), W);
        const int F = it % 10 == 0 ? 300 : 20, mpf = it % 11 == 0 ? 40 : 5;
        differ += lists_differ(off, rows, F, mpf, lim);
        const S3Lists l = s3_work_lists(off.data(), rows, F, mpf, lim);
        differ += !s3_wave_ok(F, mpf, lim) && !l.small.empty();
        nsmall += static_cast<int>(l.small.size());
        nbig += static_cast<int>(l.big.size());
    }
    CHECK(differ == 0);
    CHECK(nsmall > 1000 && nbig > 1000);
    {  // a size above kS3CountSortMax: std::stable_sort instead of the counting sort
        const vec32 off = offsets({5, kS3CountSortMax + 1, 5, 9, kS3CountSortMax + 1, 2000});
        CHECK(lists_differ(off, {0, 6}, 20, 5, lim) == 0);
        const S3Lists l = s3_work_lists(off.data(), {0, 6}, 20, 5, lim);
        CHECK((l.big == std::vector<int>{1, 4, 5}) && (l.small == std::vector<int>{3, 0, 2}));
        const vec32 at = offsets({5, kS3CountSortMax, 6, 2000});  // the largest size the counting sort takes
        CHECK(lists_differ(at, {0, 4}, 20, 5, lim) == 0);
    }
}

static void replica_cases()
{
    auto fits = [](int R, int F) { return static_cast<size_t>(R) * hist_stride(F) * 4 <= kHistReplicaBytes; };
    for (int F : {1, 64, 318, 319, 320, 10238, 10239, 16384}) {
        const int R = hist_replicas(F);
        CHECK(R >= 1 && R <= 32 && (R & (R - 1)) == 0);
        CHECK(hist_stride(F) % 2 == 1 && hist_stride(F) >= F + 1);
        // the copies fit the budget; from 10239 frames on not even one does and R stays 1 (the
        // kernel's LDS request is then the tile buffers plus that one copy)
        CHECK(fits(R, F) || (R == 1 && F >= 10239));
        CHECK(R == 32 || !fits(2 * R, F));
    }
    CHECK(hist_replicas(1) == 32 && hist_replicas(64) == 32 && hist_replicas(318) == 32);
    CHECK(hist_replicas(319) == 16 && hist_replicas(320) == 16);
    CHECK(fits(1, 10238) && !fits(1, 10239) && hist_replicas(16384) == 1);
    // the LDS the two S4 kernels ask for: tile buffers + replicas; F + 1 cumulative counts + the static arrays
    CHECK(hist_lds_bytes(318, 8192) == 8192 + 32 * 319 * 4 && hist_lds_bytes(16384, 8192) == 73732);
    CHECK(thresholds_lds_dynamic(16384) == 131080 && thresholds_lds_bytes(16384, 2128) == 133208);
    CHECK(thresholds_lds_bytes(16384, 2128) <= 160 * 1024 && hist_lds_bytes(16384, 8192) > 64 * 1024);
}

static void s6_cases()
{
    CHECK(!s6_mode(0.9).dense_obs && s6_mode(0.9).ctf == 0.9f);
    CHECK(!s6_mode(1.0).dense_obs && s6_mode(1.0).ctf == 1.0f);
    CHECK(s6_mode(0.0).dense_obs && s6_mode(-1.0).dense_obs && s6_mode(-0.0).dense_obs);
    const S6Mode m = s6_mode(std::nan(""));  // no comparison passes: sparse, and no edge
    CHECK(!m.dense_obs && std::isnan(m.ctf));

    CHECK(!s6_components_fused(0, 1) && !s6_components_fused(0, 32768));  // level 0 never
    CHECK(s6_components_fused(1, 1) && s6_components_fused(1, 32768) && !s6_components_fused(1, 32769));
    CHECK(s6_components_fused(7, 32768) && !s6_components_fused(7, 262144));
    CHECK(kFusedComponentsMaxN0 == 32768);
}

int main()
{
    frame_start_cases();
    row_cut_cases();
    work_list_cases();
    replica_cases();
    s6_cases();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
