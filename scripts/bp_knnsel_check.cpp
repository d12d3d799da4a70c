// S1 denoise k-NN candidate selection (maskclustering_amd/csrc/mc_bp_knnsel.hpp) on the CPU: the distance
// class, the class histogram's threshold, the sorting network, and the whole selection written as step 10 of
// k_bp_denoise_lds (mc_bp_denoise_lds.inl) is, against std::sort.  Built and run by tests/test_bp_knnsel_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -ffp-contract=off -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/bp_knnsel_check.cpp -o bp_knnsel_check && ./bp_knnsel_check
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <vector>

#include "mc_bp_knnsel.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);  \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;

static std::mt19937_64 rng(20240611);
static double uni() { return std::uniform_real_distribution<double>(0.0, 1.0)(rng); }

// ---- the class of a squared distance: monotone, 0 .. 15, clamped below eps2 ----
static void classes()
{
    for (double eps : {0.04, 0.1, 0.0123}) {
        const double eps2 = eps * eps, s = knn_scale(eps2);
        CHECK(knn_class(0.0, s) == 0u);
        for (int i = 0; i < 1000000; i++) {
            const double d2 = uni() * eps2;
            if (!(d2 < eps2)) continue;
            const unsigned c = knn_class(d2, s);
            CHECK(c <= 15u);
            const double up = std::nextafter(d2, 1.0), dn = std::nextafter(d2, -1.0);
            CHECK(knn_class(up, s) >= c);
            if (dn >= 0.0) CHECK(knn_class(dn, s) <= c);
        }
        // class boundaries: across each multiple of eps2 / 16 the class steps by at most one and never back
        for (int k = 1; k <= 16; k++) {
            double d2 = eps2 * k / 16.0;
            for (int j = 0; j < 8; j++) d2 = std::nextafter(d2, 0.0);
            unsigned prev = knn_class(d2, s);
            for (int j = 0; j < 16; j++) {
                d2 = std::nextafter(d2, 1.0);
                const unsigned c = knn_class(d2, s);
                CHECK(c >= prev && c <= prev + 1u && c <= 15u);
                prev = c;
            }
        }
        // just below eps2: the clamp (d2 * s may round to 16)
        double d2 = eps2;
        for (int j = 0; j < 64; j++) {
            d2 = std::nextafter(d2, 0.0);
            CHECK(knn_class(d2, s) == 15u);
        }
        CHECK(knn_class(eps2, s) == 15u);
    }
}

// ---- threshold against a cumulative scan ----
static int threshold_ref(const int (&cnt)[kKnnClasses], int kk)
{
    int cum = 0;
    for (int c = 0; c < kKnnClasses; c++) {
        cum += cnt[c];
        if (cum >= kk) return c;
    }
    return -1;
}
static void check_hist(const int (&cnt)[kKnnClasses], int kk)
{
    KnnHist h;
    // interleave the classes' entries and a few uncounted ones (on = 0)
    int left[kKnnClasses], total = 0;
    for (int c = 0; c < kKnnClasses; c++) total += left[c] = cnt[c];
    while (total > 0) {
        const unsigned c = static_cast<unsigned>(rng() % kKnnClasses);
        h.add(static_cast<unsigned>(rng() % kKnnClasses), 0u);
        if (left[c] > 0) {
            h.add(c, 1u);
            left[c]--;
            total--;
        }
    }
    for (int c = 0; c < kKnnClasses; c++) CHECK(h.count(static_cast<unsigned>(c)) == static_cast<unsigned>(cnt[c]));
    CHECK(knn_threshold(h, kk) == threshold_ref(cnt, kk));
}
static void thresholds()
{
    for (int kk : {1, 5, 20, 64}) {
        for (int c = 0; c < kKnnClasses; c++) {  // all entries in one class: below, at and above kk, and 64
            for (int n : {0, kk - 1, kk, kk + 1, 64}) {
                if (n < 0 || n > 64) continue;
                int cnt[kKnnClasses] = {};
                cnt[c] = n;
                check_hist(cnt, kk);
            }
        }
        for (int i = 0; i < 20000; i++) {  // random histograms of total 0 .. 64 (totals below, at and above kk)
            int cnt[kKnnClasses] = {};
            const int total = i % 3 == 0 ? kk : i % 3 == 1 ? static_cast<int>(rng() % 65) : std::max(0, kk - 1 - static_cast<int>(rng() % 3));
            const int spread = 1 + static_cast<int>(rng() % kKnnClasses);
            for (int j = 0; j < total; j++) cnt[(rng() % spread) * (kKnnClasses / spread) % kKnnClasses]++;
            check_hist(cnt, kk);
        }
    }
}

// ---- the network: every 0-1 input, bit-sliced (64 inputs per word) ----
static void network()
{
    CHECK(kKnnNetList.n > 0 && kKnnNetList.n <= 192);
    for (int i = 0; i < kKnnNetList.n; i++) CHECK(kKnnNetList.a[i] < kKnnNetList.b[i] && kKnnNetList.b[i] < kKnnNet);
    static_assert(kKnnNet >= 6 && kKnnNet <= 32, "2^kKnnNet inputs in blocks of 64");
    const uint64_t low[6] = {0xAAAAAAAAAAAAAAAAull, 0xCCCCCCCCCCCCCCCCull, 0xF0F0F0F0F0F0F0F0ull,
                             0xFF00FF00FF00FF00ull, 0xFFFF0000FFFF0000ull, 0xFFFFFFFF00000000ull};
    unsigned long long fails = 0;
    for (uint64_t blk = 0; blk < (1ull << (kKnnNet - 6)); blk++) {
        uint64_t d[kKnnNet];
        for (int l = 0; l < kKnnNet; l++) d[l] = l < 6 ? low[l] : ((blk >> (l - 6)) & 1ull) ? ~0ull : 0ull;
        knn_net_sort(d, [](uint64_t &lo, uint64_t &hi) {
            const uint64_t x = lo, y = hi;
            lo = x & y;  // the minimum of two bits
            hi = x | y;
        });
        // sorted: line l <= line l + 1 in every input
        for (int l = 0; l + 1 < kKnnNet; l++) fails += (d[l] & ~d[l + 1]) != 0;
    }
    CHECK(fails == 0);
    // (comparators only exchange, so a sorted output is the sorted input.)  The outputs the pass reads: the first
    // kKnnOut equal the sorted input's first kKnnOut, on values with ties and +max padding
    for (int i = 0; i < 20000; i++) {
        double d[kKnnNet], ref[kKnnNet];
        for (int l = 0; l < kKnnNet; l++) ref[l] = d[l] = (rng() % 4 == 0) ? DBL_MAX : static_cast<double>(rng() % 12) * 0.125;
        knn_net_sort(d, [](double &lo, double &hi) {
            const double x = lo, y = hi;
            lo = __builtin_fmin(x, y);
            hi = __builtin_fmax(x, y);
        });
        std::sort(ref, ref + kKnnNet);
        for (int l = 0; l < kKnnOut; l++) CHECK(std::memcmp(&d[l], &ref[l], 8) == 0);
    }
}

// ---- the whole selection, as the list pass runs it ----
static void selection()
{
    const int kk = kKnnOut;
    const double eps = 0.04, eps2 = eps * eps, s = knn_scale(eps2);
    int over_net = 0, exact = 0, deferred = 0;
    for (int it = 0; it < 60000; it++) {
        const int cnt = 20 + static_cast<int>(rng() % 45);  // 20 .. 64 entries
        const int mode = it % 4;  // 0: spread, 1: lattice (many ties), 2: one tight shell (a large selected set), 3: few kept
        std::vector<double> d2(cnt);
        std::vector<int> kept(cnt);
        for (int k = 0; k < cnt; k++) {
            double v;
            if (mode == 1) v = static_cast<double>(rng() % 9) * 1e-4 + static_cast<double>(rng() % 3) * 1e-4;
            else if (mode == 2) v = 0.0005 + 1e-6 * static_cast<double>(rng() % 40);
            else v = uni() * eps2;
            if (!(v < eps2)) v = 0.0;
            d2[k] = v;
            kept[k] = mode == 3 ? (rng() % 2 == 0) : (rng() % 8 != 0);
        }
        // class -> histogram -> pm
        KnnHist hist;
        uint64_t mall = 0, pm = 0;
        for (int k = 0; k < cnt; k++) {
            const uint32_t on = kept[k] ? 1u : 0u;
            mall |= static_cast<uint64_t>(on) << k;
            hist.add(knn_class(d2[k], s), on);
        }
        const int found = __builtin_popcountll(mall);
        const int cstar = knn_threshold(hist, kk);
        CHECK((cstar < 0) == (found < kk));
        if (found < kk) {  // the ring queue's
            deferred++;
            continue;
        }
        for (int k = 0; k < cnt; k++) pm |= static_cast<int>(knn_class(d2[k], s)) <= cstar ? 1ull << k : 0ull;
        pm &= mall;
        const int sel = __builtin_popcountll(pm);
        CHECK(sel >= kk);
        over_net += sel > kKnnNet;
        exact += sel == kk;
        // one round into the network's array, then the leftovers
        double best[kKnnNet];
        for (int u = 0; u < kKnnNet; u++) {
            const int b = pm ? __builtin_ctzll(pm) : -1;
            pm &= pm - 1;
            best[u] = b >= 0 ? d2[b] : DBL_MAX;
        }
        knn_net_sort(best, [](double &lo, double &hi) {
            const double x = lo, y = hi;
            lo = __builtin_fmin(x, y);
            hi = __builtin_fmax(x, y);
        });
        while (pm) {
            const int b = __builtin_ctzll(pm);
            pm &= pm - 1;
            knn_insert<kKnnOut>(
                best, d2[b], [](double x, double y) { return __builtin_fmin(x, y); },
                [](double x, double y) { return __builtin_fmax(x, y); });
        }
        double sum = 0.0;
        for (int k = 0; k < kk; k++) sum = sum + std::sqrt(best[k]);
        // the reference: every kept entry, sorted
        std::vector<double> ref;
        for (int k = 0; k < cnt; k++)
            if (kept[k]) ref.push_back(d2[k]);
        std::sort(ref.begin(), ref.end());
        for (int k = 0; k < kk; k++) CHECK(std::memcmp(&best[k], &ref[k], 8) == 0);
        std::vector<double> roots(kk);
        for (int k = 0; k < kk; k++) roots[k] = std::sqrt(ref[k]);
        const double rsum = std::accumulate(roots.begin(), roots.end(), 0.0);
        CHECK(std::memcmp(&sum, &rsum, 8) == 0);
    }
    CHECK(over_net > 100);  // the leftover path
    CHECK(exact > 100);     // a selected set of exactly k
    CHECK(deferred > 100);  // fewer than k kept entries
    printf("selection: over_net=%d exact=%d deferred=%d\n", over_net, exact, deferred);
}

int main()
{
    classes();
    thresholds();
    network();
    selection();
    printf("net=%d comparators=%d bad=%d\n", kKnnNet, kKnnNetList.n, bad);
    return bad ? 1 : 0;
}
