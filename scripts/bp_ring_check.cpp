// S1 denoise ring search (maskclustering_amd/csrc/mc_bp_ring.hpp) on the CPU: the enumeration of the two rings'
// cells, the mask, the gap bound, and the search written as k_bp_knn_ring (mc_bp_denoise.inl) is (mark and walk
// of ring 0, the test for being settled, mark and walk of the shell, the test again) over a hashed grid built as
// the class kernel builds it, against a brute-force scan.  Built and run by tests/test_bp_ring_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -ffp-contract=off -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/bp_ring_check.cpp -o bp_ring_check && ./bp_ring_check
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "mc_bp_ring.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);  \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;

constexpr int K = 20;  // kBpKnnMax
constexpr unsigned long long kKept = 1ull << 63;

static std::mt19937_64 rng(20250317);
static double uni() { return std::uniform_real_distribution<double>(0.0, 1.0)(rng); }

static unsigned long long bits(double v)
{
    unsigned long long b;
    memcpy(&b, &v, 8);
    return b;
}

// ---- the enumeration: every cell of a ring exactly once; the mask ----
static void enumeration()
{
    for (int ring = 0; ring < 2; ring++) {
        const int R = ring + 1;
        std::set<std::tuple<int, int, int>> seen;
        for (int i = 0; i < ring_cells(ring); i++) {
            int dx, dy, dz;
            ring_cell(ring, i, dx, dy, dz);
            const int c = std::max(std::abs(dx), std::max(std::abs(dy), std::abs(dz)));
            CHECK(ring == 0 ? c <= 1 : c == 2);
            CHECK(c <= R);
            CHECK(seen.insert({dx, dy, dz}).second);
        }
        CHECK(static_cast<int>(seen.size()) == (ring == 0 ? 27 : 98));
    }
    int dx, dy, dz;
    ring_cell(0, 0, dx, dy, dz);
    CHECK(dx == 0 && dy == 0 && dz == 0);  // the own cell first
    CHECK(ring_cells(0) == 27 && ring_cells(1) == 98 && kRingMarkGroup >= 8 && kRingMarkGroup <= 16);
    // the mask: set bits come back ascending, once each; unset and off bits do not
    for (int t = 0; t < 2000; t++) {
        RingMask m;
        std::vector<int> want;
        const double p = uni();
        for (int i = 0; i < kRingShell + kRingMarkGroup; i++) {
            const bool on = i < kRingShell && uni() < p;
            m.set(i, on);
            if (on) want.push_back(i);
        }
        for (int i = 0; i < kRingShell; i++) CHECK(m.test(i) == (std::find(want.begin(), want.end(), i) != want.end()));
        std::vector<int> got;
        while (m.any()) got.push_back(m.pop());
        CHECK(got == want);
    }
}

// ---- a slot's grid as the class kernel leaves it: records sorted by bucket, cell key and kept bit in w ----
struct Rec {
    double x, y, z, w;
};
static unsigned hash3(int x, int y, int z)
{
    return static_cast<unsigned>(x) * 0x9E3779B1u + static_cast<unsigned>(y) * 0x85EBCA77u +
           static_cast<unsigned>(z) * 0xC2B2AE3Du;
}
static unsigned long long pack3(int x, int y, int z)
{
    return (static_cast<unsigned long long>(x) << 42) | (static_cast<unsigned long long>(y) << 21) |
           static_cast<unsigned long long>(z);
}
struct Grid {
    std::vector<Rec> pt;
    std::vector<int> bs;
    unsigned nb = 1;
    double mn[3] = {0, 0, 0};
    mutable long reads = 0;

    unsigned bucket(int x, int y, int z) const
    {
        return static_cast<unsigned>((static_cast<unsigned long long>(hash3(x, y, z)) * nb) >> 32);
    }
    int start(unsigned b) const { return bs.at(b); }
    const Rec &rec(int q) const
    {
        reads++;
        return pt.at(static_cast<size_t>(q));
    }
    unsigned long long key(const Rec &p) const { return bits(p.w); }
    unsigned long long cell_key(int x, int y, int z) const { return pack3(x, y, z) | kKept; }
};

struct Pt {
    double x, y, z;
    bool kept;
};

static void cell_of(const Grid &g, const Pt &p, double ce, int c[3])
{
    c[0] = static_cast<int>(std::floor((p.x - g.mn[0]) / ce));
    c[1] = static_cast<int>(std::floor((p.y - g.mn[1]) / ce));
    c[2] = static_cast<int>(std::floor((p.z - g.mn[2]) / ce));
}

static Grid build(const std::vector<Pt> &P, double ce, double half_voxel, unsigned nb)
{
    Grid g;
    g.nb = nb;
    for (int a = 0; a < 3; a++) g.mn[a] = DBL_MAX;
    for (const Pt &p : P) {
        g.mn[0] = std::min(g.mn[0], p.x);
        g.mn[1] = std::min(g.mn[1], p.y);
        g.mn[2] = std::min(g.mn[2], p.z);
    }
    for (int a = 0; a < 3; a++) g.mn[a] -= half_voxel;
    std::vector<unsigned> b(P.size());
    g.bs.assign(nb + 1, 0);
    for (size_t i = 0; i < P.size(); i++) {
        int c[3];
        cell_of(g, P[i], ce, c);
        b[i] = g.bucket(c[0], c[1], c[2]);
        g.bs[b[i] + 1]++;
    }
    for (unsigned k = 0; k < nb; k++) g.bs[k + 1] += g.bs[k];
    std::vector<int> at(g.bs.begin(), g.bs.end() - 1);
    g.pt.resize(P.size());
    for (size_t i = 0; i < P.size(); i++) {
        int c[3];
        cell_of(g, P[i], ce, c);
        const unsigned long long w = pack3(c[0], c[1], c[2]) | (P[i].kept ? kKept : 0ull);
        Rec r{P[i].x, P[i].y, P[i].z, 0.0};
        memcpy(&r.w, &w, 8);
        g.pt[static_cast<size_t>(at[b[i]]++)] = r;
    }
    return g;
}

static void insert(double (&a)[K], double v)
{
    if (!(v < a[K - 1])) return;
    int q = K - 1;
    for (; q > 0 && v < a[q - 1]; q--) a[q] = a[q - 1];
    a[q] = v;
}

static long n_pts = 0, n_r1 = 0, n_r2 = 0, n_all = 0, n_ties = 0, n_skipped = 0;

// every kept point of the cloud searches as a deferred point does
static void search_cloud(const std::vector<Pt> &P, double eps, double half_voxel, unsigned nb)
{
    const double ce = 1.01 * eps, sl = 1e-9 * ce;
    const Grid g = build(P, ce, half_voxel, nb);
    for (const Pt &a : P) {
        if (!a.kept) continue;
        n_pts++;
        int c[3];
        cell_of(g, a, ce, c);
        const double ox = std::fmin(std::fmax(a.x - g.mn[0] - c[0] * ce, 0.0), ce);
        const double oy = std::fmin(std::fmax(a.y - g.mn[1] - c[1] * ce, 0.0), ce);
        const double oz = std::fmin(std::fmax(a.z - g.mn[2] - c[2] * ce, 0.0), ce);
        const RingWhere w{{c[0], c[1], c[2]}, {ox, oy, oz}};
        // brute force: every kept point's d2 with its cell offset
        struct Cand {
            double d2;
            int d[3];
        };
        std::vector<Cand> all;
        for (const Pt &p : P) {
            if (!p.kept) continue;
            int pc[3];
            cell_of(g, p, ce, pc);
            const double ex = a.x - p.x, ey = a.y - p.y, ez = a.z - p.z;
            all.push_back({((ex * ex) + (ey * ey)) + (ez * ez), {pc[0] - c[0], pc[1] - c[1], pc[2] - c[2]}});
        }
        auto smallest = [&](int R, double (&out)[K]) {  // the K smallest d2 among the cells within R
            std::vector<double> v;
            for (const Cand &q : all)
                if (std::max(std::abs(q.d[0]), std::max(std::abs(q.d[1]), std::abs(q.d[2]))) <= R) v.push_back(q.d2);
            std::sort(v.begin(), v.end());
            for (int k = 0; k < K; k++) out[k] = k < static_cast<int>(v.size()) ? v[static_cast<size_t>(k)] : DBL_MAX;
        };
        // the gap of a cell is a lower bound of the computed distance to every point in it
        for (const Cand &q : all) {
            if (std::max(std::abs(q.d[0]), std::max(std::abs(q.d[1]), std::abs(q.d[2]))) > 2) continue;
            CHECK(ring_gap2(q.d[0], q.d[1], q.d[2], ox, oy, oz, ce, sl) <= q.d2);
        }
        double best[K];
        for (double &b : best) b = DBL_MAX;
        int found = 0;
        bool done = false;
        for (int ring = 0; ring < 2 && !done; ring++) {
            const RingMask m = ring_mark(g, ring, w, ce, sl, best[K - 1]);
            // a cell that holds a point below the final k-th distance of this ring is marked
            double want[K];
            smallest(ring + 1, want);
            for (int i = 0; i < ring_cells(ring); i++) {
                int dx, dy, dz;
                ring_cell(ring, i, dx, dy, dz);
                for (const Cand &q : all)
                    if (q.d[0] == dx && q.d[1] == dy && q.d[2] == dz && q.d2 < want[K - 1]) CHECK(m.test(i));
            }
            const long before = g.reads;
            ring_walk(
                g, ring, m, w, a.x, a.y, a.z, ce, sl, [&] { return best[K - 1]; },
                [&](double d2, bool on) {
                    if (!on) return;
                    insert(best, d2);
                    found++;
                });
            if (ring == 1 && g.reads == before) n_skipped++;
            for (int k = 0; k < K; k++) CHECK(bits(best[k]) == bits(want[k]));
            const double reach = static_cast<double>(ring + 1) * ce;
            done = found >= K && best[K - 1] < reach * reach * (1.0 - 1e-9);
            if (done) (ring == 0 ? n_r1 : n_r2)++;
        }
        double full[K];
        smallest(1 << 30, full);
        if (done) {
            for (int k = 0; k < K; k++) CHECK(bits(best[k]) == bits(full[k]));
            if (best[K - 1] == best[K - 2]) n_ties++;
        } else {
            n_all++;
        }
    }
}

static std::vector<Pt> cloud(int kind, int n, double eps)
{
    std::vector<Pt> P;
    const double sp = eps * (0.15 + 0.5 * uni());  // point spacing
    const double o[3] = {uni() * 4 - 2, uni() * 4 - 2, uni() * 4 - 2};
    const int side = std::max(2, static_cast<int>(std::ceil(std::sqrt(static_cast<double>(n)))));
    for (int i = 0; i < n; i++) {
        Pt p{0, 0, 0, true};
        switch (kind) {
        case 0:  // random in a box
            p = {o[0] + uni() * sp * 6, o[1] + uni() * sp * 6, o[2] + uni() * sp * 6, true};
            break;
        case 1:  // an exact lattice wall (multiples of 2^-8: squared distances tie)
            p = {(i % side) * 3.0 / 256, (i / side) * 3.0 / 256, 0.75, true};
            break;
        case 2:  // a tilted, jittered surface patch
        {
            const double u = (i % side) * sp, v = (i / side) * sp;
            p = {o[0] + u, o[1] + v, o[2] + 0.3 * u - 0.2 * v + 0.05 * sp * uni(), true};
            break;
        }
        case 3:  // an edge strip: two rows
            p = {o[0] + (i / 2) * sp, o[1] + (i % 2) * sp * 0.7, o[2] + 0.01 * sp * uni(), true};
            break;
        default:  // a lattice cube
        {
            const int s3 = std::max(2, static_cast<int>(std::ceil(std::cbrt(static_cast<double>(n)))));
            p = {(i % s3) * 5.0 / 512, ((i / s3) % s3) * 5.0 / 512, (i / (s3 * s3)) * 5.0 / 512 + 0.5, true};
        }
        }
        P.push_back(p);
    }
    if (uni() < 0.5)  // some points the class filter dropped: in the grid, never neighbours
        for (Pt &p : P) p.kept = uni() < 0.85;
    return P;
}

int main()
{
    enumeration();
    const double eps = 0.04;
    for (int kind = 0; kind < 5; kind++)
        for (int t = 0; t < 60; t++) {
            const int n = t < 30 ? 20 + static_cast<int>(uni() * 21) : 60 + static_cast<int>(uni() * 500);
            const std::vector<Pt> P = cloud(kind, n, eps);
            // as the class kernel sizes it (2 n), and far fewer buckets than a ring has cells
            for (unsigned nb : {2u * static_cast<unsigned>(n), 7u, 1u}) {
                if (nb < 8u && n > 120) continue;
                search_cloud(P, eps, 0.0125, nb);
            }
        }
    CHECK(n_r1 > 100 && n_r2 > 100 && n_all > 100 && n_ties > 10 && n_skipped > 0);
    printf("points=%ld r1=%ld r2=%ld cloud=%ld ties=%ld shell_walks_empty=%ld bad=%d\n", n_pts, n_r1, n_r2, n_all, n_ties,
           n_skipped, bad);
    return bad ? 1 : 0;
}
