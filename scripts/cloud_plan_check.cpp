// cloud_plan_check.cpp — the host decisions of the scene point cloud fusion (maskclustering_amd/csrc/mc_cloud_plan.hpp)
// checked on the CPU: the flush schedule against the reference's loop written out, the table size, the
// byte count and the refusals with their messages, the extent rule at 2^21 - 1 and 2^21 voxels, the
// voxel index, and the upward bitonic network of the per-voxel sort for every length up to 300 and
// some around the class thresholds.  A stand-alone program (tests/test_cloud_plan_cpu.py builds it
// with the address and undefined-behaviour sanitizers); prints bad=<failures>.
#include <algorithm>
#include <cstdio>
#include <random>
#include <vector>

#include "mc_cloud_plan.hpp"

static int bad = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            bad++;                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
        }                                                         \
    } while (0)

using Sched = std::vector<std::pair<int, int>>;

// tasmap2mct_format.py:255-280, frames only
static Sched reference_loop(int F, int B)
{
    Sched out;
    std::vector<int> buffer;
    for (int i = 0; i < F; i++) {
        buffer.push_back(i);
        if ((i + 1) % B == 0) {
            out.emplace_back(buffer.front(), buffer.back() + 1);
            buffer.clear();
        }
    }
    if (!buffer.empty()) out.emplace_back(buffer.front(), buffer.back() + 1);
    return out;
}

static void sort_by_network(std::vector<int> &a)
{
    const int64_t n = static_cast<int64_t>(a.size());
    for (int64_t k = 2; (k >> 1) < n; k <<= 1)
        for (int64_t j = 0, next = k >> 2;; j = next, next >>= 1) {
            std::vector<char> touched(a.size(), 0);
            for (int64_t i = 0; i < n; i++) {
                const int64_t l = mc::cloud_sort_partner(i, k, j, n);
                if (l < 0) continue;
                CHECK(l > i && l < n && !touched[i] && !touched[l]);  // a step's pairs are disjoint: no race
                touched[i] = touched[l] = 1;
                if (a[i] > a[l]) std::swap(a[i], a[l]);
            }
            if (next < 1) break;
        }
}

int main()
{
    // the schedule
    CHECK((mc::cloud_flush_schedule(7, 3) == Sched{{0, 3}, {3, 6}, {6, 7}}));
    CHECK((mc::cloud_flush_schedule(6, 3) == Sched{{0, 3}, {3, 6}}));
    CHECK((mc::cloud_flush_schedule(2, 3) == Sched{{0, 2}}));
    CHECK((mc::cloud_flush_schedule(3, 1) == Sched{{0, 1}, {1, 2}, {2, 3}}));
    CHECK(mc::cloud_flush_schedule(0, 3).empty());
    CHECK(mc::cloud_flush_schedule(5, 0).empty());
    for (int F = 0; F <= 40; F++)
        for (int B = 1; B <= 12; B++) CHECK(mc::cloud_flush_schedule(F, B) == reference_loop(F, B));

    // the table: a power of two, two entries a point, 64 at least
    CHECK(mc::cloud_table_size(0) == 64 && mc::cloud_table_size(32) == 64 && mc::cloud_table_size(33) == 128);
    CHECK(mc::cloud_table_size((int64_t(1) << 31) - 1) == (uint64_t(1) << 32));
    for (int64_t n : {1ll, 1000ll, 4097ll, 30000000ll}) {
        const uint64_t t = mc::cloud_table_size(n);
        CHECK((t & (t - 1)) == 0 && t >= 2 * static_cast<uint64_t>(n) && (t == 64 || t / 2 < 2 * static_cast<uint64_t>(n)));
        CHECK((uint64_t(1) << mc::cloud_table_log2(t)) == t);
        CHECK(mc::cloud_hash(0x123456789abcull * n, mc::cloud_table_log2(t)) < t);
    }

    // bytes and the refusals
    CHECK(mc::cloud_stage_bytes(2, 0) == 2 * 24 + 16 * 64 + 16 * 3 + 12 * 3 + 2 * 24 + mc::kCloudSlack);
    CHECK(mc::cloud_stage_bytes(2, 24) == mc::cloud_stage_bytes(2, 0) + 2 * 48);
    CHECK(mc::cloud_stage_bytes(1000, 3) < mc::cloud_stage_bytes(1001, 3));
    CHECK(mc::cloud_byte_budget(12345, 1 << 30) == 12345 && mc::cloud_byte_budget(0, 1000) == 800);
    std::string why;
    CHECK(mc::cloud_check_count(1000, 3, 0, int64_t(1) << 30, &why) == mc::kCloudAccept);
    CHECK(mc::cloud_check_count(int64_t(1) << 31, 3, 0, int64_t(1) << 62, &why) == mc::kCloudUnsupported &&
          why.find("2^31") != std::string::npos);
    CHECK(mc::cloud_check_count((int64_t(1) << 31) - 1, 3, 0, int64_t(1) << 62, &why) == mc::kCloudAccept);
    const int64_t need = mc::cloud_stage_bytes(1000, 3) + 77;
    CHECK(mc::cloud_check_count(1000, 3, 77, need, &why) == mc::kCloudAccept);
    CHECK(mc::cloud_check_count(1000, 3, 77, need - 1, &why) == mc::kCloudUnsupported &&
          why.find(std::to_string(need) + " bytes") != std::string::npos);

    // the extent: the largest index is the maximum's; 2^21 - 1 is accepted, 2^21 refused
    {
        const double vs = 0.5;
        const double mn[3] = {0, 0, 0};
        // index of p = floor((p + vs / 2) / vs): p = (2^21 - 1) * vs gives 2^21 - 1, p = 2^21 * vs gives 2^21
        const double ok[3] = {(double)((1 << 21) - 1) * vs, 0, 0}, over[3] = {0, 0, (double)(1 << 21) * vs};
        CHECK(mc::cloud_voxel_index(ok[0], mc::cloud_vmin(0, vs), vs) == (1 << 21) - 1);
        CHECK(mc::cloud_voxel_index(over[2], mc::cloud_vmin(0, vs), vs) == (1 << 21));
        CHECK(mc::cloud_check_extent(mn, ok, true, vs, &why) == mc::kCloudAccept);
        CHECK(mc::cloud_check_extent(mn, over, true, vs, &why) == mc::kCloudUnsupported && why.find("2^21") != std::string::npos);
        CHECK(mc::cloud_check_extent(mn, ok, false, vs, &why) == mc::kCloudInvalid);
        const double far_mn[3] = {-1e4, -1e4 - 3, -1e4}, far_mx[3] = {-1e4 + 2, -1e4, -1e4 + 1};
        CHECK(mc::cloud_check_extent(far_mn, far_mx, true, 0.005, &why) == mc::kCloudAccept);
    }
    // the key keeps the three indices apart and never is the empty mark
    CHECK(mc::cloud_pack_key(1, 2, 3) == ((uint64_t(1) << 42) | (uint64_t(2) << 21) | 3));
    CHECK(mc::cloud_pack_key((1 << 21) - 1, (1 << 21) - 1, (1 << 21) - 1) == (uint64_t(1) << 63) - 1);
    CHECK(mc::cloud_pack_key((1 << 21) - 1, (1 << 21) - 1, (1 << 21) - 1) != mc::kCloudEmptyKey);
    CHECK(mc::cloud_voxel_index(0.0, mc::cloud_vmin(0.0, 0.005), 0.005) == 0);
    CHECK(mc::cloud_voxel_index(0.0026, mc::cloud_vmin(0.0, 0.005), 0.005) == 1);

    // the network sorts every length
    std::mt19937 rng(7);
    std::vector<int> lengths;
    for (int n = 0; n <= 300; n++) lengths.push_back(n);
    for (int n : {mc::kCloudThreadMax + 1, 1023, 1025, mc::kCloudLdsMax - 1, mc::kCloudLdsMax, mc::kCloudLdsMax + 1, 5000})
        lengths.push_back(n);
    for (int n : lengths)
        for (int rep = 0; rep < (n <= 300 ? 3 : 1); rep++) {
            std::vector<int> a(n);
            for (int i = 0; i < n; i++) a[i] = rep == 2 ? n - i : static_cast<int>(rng() % 1000000) * 2 + (i & 1);
            std::vector<int> want = a;
            std::sort(want.begin(), want.end());
            sort_by_network(a);
            CHECK(a == want);
        }
    CHECK(mc::kCloudThreadMax < mc::kCloudLdsMax && mc::kCloudFoldChunk <= 256);
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
