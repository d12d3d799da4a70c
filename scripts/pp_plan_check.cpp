// Post-processing host decisions (maskclustering_amd/csrc/mc_pp_plan.hpp) on the CPU: worked cases of
// every function, and the greedy merge over shuffled decision lists against a dense restatement of
// post_process.py:14-29.  Built and run by tests/test_pp_plan_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/pp_plan_check.cpp -o pp_plan_check && ./pp_plan_check
#include <cstdio>
#include <random>

#include "mc_pp_plan.hpp"

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

static bool same_items(const std::vector<PPInt2> &a, const std::vector<PPInt2> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++)
        if (a[i].x != b[i].x || a[i].y != b[i].y) return false;
    return true;
}

static void big_items()
{
    static_assert(sizeof(PPInt2) == 8, "two packed ints, as the kernels' int2");
    std::vector<PPInt2> items{{7, 7}};
    {  // sizes 1300, 600, 512, 10: a size equal to big_min is not big
        const int64_t off[] = {0, 1300, 1900, 2412, 2422};
        const int32_t order[] = {0, 1, 2, 3};
        CHECK(pp_big_items(off, order, 4, 512, items) == 2);
        CHECK(same_items(items, {{0, 0}, {0, 512}, {0, 1024}, {1, 0}, {1, 512}}));
        CHECK(pp_big_items(off, order, 4, 1300, items) == 0 && items.empty());
        CHECK(pp_big_items(off, order, 4, 9, items) == 4);  // all nodes big
        CHECK(same_items(items, {{0, 0}, {0, 512}, {0, 1024}, {1, 0}, {1, 512}, {2, 0}, {3, 0}}));
    }
    {  // the order decides, not the node index: sizes 10, 1025 in size order
        const int64_t off[] = {0, 10, 1035};
        const int32_t order[] = {1, 0};
        CHECK(pp_big_items(off, order, 2, 512, items) == 1);
        CHECK(same_items(items, {{1, 0}, {1, 512}, {1, 1024}}));
    }
    const int64_t off0[] = {0};
    CHECK(pp_big_items(off0, nullptr, 0, 512, items) == 0 && items.empty());  // N == 0
}

static void kept_and_final()
{
    // five objects of nodes 0, 0, 1, 1, 2: object 1 kept no point, object 3 has one mask only
    const vec32 nv{4, 0, 7, 3, 2}, nm{2, 3, 5, 1, 2};
    std::vector<double> box(30);
    for (int i = 0; i < 30; i++) box[i] = i;
    const PPKept k = pp_kept_objects(5, nv.data(), nm.data(), box.data());
    CHECK((k.kidx == vec32{0, -1, 1, -1, 2}));
    CHECK((k.kept == vec32{0, 2, 4}));
    CHECK((k.klen == vec32{4, 7, 2}));
    CHECK((k.kbox == std::vector<double>{0, 1, 2, 3, 4, 5, 12, 13, 14, 15, 16, 17, 24, 25, 26, 27, 28, 29}));
    const PPKept none = pp_kept_objects(0, nullptr, nullptr, nullptr);
    CHECK(none.kidx.empty() && none.kept.empty() && none.klen.empty() && none.kbox.empty());

    // kept object 2 merged away: states 2, 0, 1, 0, 2
    const std::vector<uint8_t> state{2, 0, 1, 0, 2};
    const vec32 node{0, 0, 1, 1, 2};
    vec32 fslot{9}, fin{9}, fin_node{9};
    std::vector<int64_t> opoff{9, 9}, omoff;
    pp_final_tables(state, node, nv.data(), nm.data(), fslot, fin, fin_node, opoff, omoff);
    CHECK((fslot == vec32{0, -1, -1, -1, 1}));
    CHECK((fin == vec32{0, 4}));
    CHECK((fin_node == vec32{0, 2}));
    CHECK((opoff == std::vector<int64_t>{0, 4, 6}));
    CHECK((omoff == std::vector<int64_t>{0, 2, 4}));
    pp_final_tables({}, {}, nullptr, nullptr, fslot, fin, fin_node, opoff, omoff);
    CHECK(fslot.empty() && fin.empty() && fin_node.empty());
    CHECK((opoff == std::vector<int64_t>{0}) && (omoff == std::vector<int64_t>{0}));
    CHECK(static_cast<int64_t>(kPPMaxKept) * kPPMaxKept <= INT32_MAX);
    CHECK(static_cast<int64_t>(kPPMaxKept + 1) * (kPPMaxKept + 1) > INT32_MAX);
}

// dec[i * K + j], j > i: 0 no decision, 1 invalidates i (:27), 2 invalidates j (:29)
static std::vector<uint8_t> dense_merge(int K, const std::vector<uint8_t> &dec)
{
    std::vector<uint8_t> invalid(K, 0);
    for (int i = 0; i < K; i++) {
        if (invalid[i]) continue;
        for (int j = i + 1; j < K; j++) {
            if (invalid[j]) continue;
            if (dec[i * K + j] == 1) invalid[i] = 1;
            else if (dec[i * K + j] == 2) invalid[j] = 1;
        }
    }
    return invalid;
}

static std::vector<PPInt2> decision_list(int K, const std::vector<uint8_t> &dec)
{
    std::vector<PPInt2> d;
    for (int i = 0; i < K; i++)
        for (int j = i + 1; j < K; j++)
            if (dec[i * K + j]) d.push_back({i, dec[i * K + j] == 1 ? -1 - j : j});
    return d;
}

static void greedy_merge()
{
    using flags = std::vector<uint8_t>;
    {  // row 0's flag is read once: (0, 2) still applies after (0, 1) invalidated object 0
        std::vector<PPInt2> d{{0, 2}, {0, -1 - 1}};
        flags inv(3, 0);
        pp_greedy_merge(d, inv);
        CHECK((inv == flags{1, 0, 1}));
    }
    {  // row 1 was invalidated by row 0: its decisions are skipped, object 2 and 3 stay
        std::vector<PPInt2> d{{1, -1 - 3}, {1, 2}, {0, 1}};
        flags inv(4, 0);
        pp_greedy_merge(d, inv);
        CHECK((inv == flags{0, 1, 0, 0}));
    }
    {  // an invalid j is skipped: (1, 2) would invalidate object 1, but row 0 took object 2 first
        std::vector<PPInt2> d{{1, -1 - 2}, {0, 2}};
        flags inv(3, 0);
        pp_greedy_merge(d, inv);
        CHECK((inv == flags{0, 0, 1}));
    }
    {
        std::vector<PPInt2> d;
        flags inv;
        pp_greedy_merge(d, inv);  // nothing kept
        flags one(1, 0);
        pp_greedy_merge(d, one);
        CHECK(one[0] == 0);
    }
    std::mt19937 rng(20240607);
    int differ = 0, nonzero = 0;
    for (int it = 0; it < 2000; it++) {
        const int K = 1 + static_cast<int>(rng() % 40);
        const double density = 0.5 * (it % 21) / 20.0;  // 0 .. 0.5
        std::vector<uint8_t> dec(static_cast<size_t>(K) * K, 0);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (int i = 0; i < K; i++)
            for (int j = i + 1; j < K; j++)
                if (u(rng) < density) dec[i * K + j] = 1 + rng() % 2;
        std::vector<PPInt2> d = decision_list(K, dec);
        std::shuffle(d.begin(), d.end(), rng);
        flags inv(K, 0);
        pp_greedy_merge(d, inv);
        const flags want = dense_merge(K, dec);
        differ += inv != want;
        for (uint8_t f : want) nonzero += f;
    }
    CHECK(differ == 0);
    CHECK(nonzero > 2000);  // the cases do merge
}

int main()
{
    big_items();
    kept_and_final();
    greedy_merge();
    printf("bad=%d\n", bad);
    return bad ? 1 : 0;
}
