// S1 ball query cell arithmetic (maskclustering_amd/csrc/mc_bp_qcell.hpp) on the CPU: the cell range of a
// float32 box holds the cell of every point strictly inside it (random and border-valued floats, the
// kCellBias clamps included), and the numbering of a box's cells is a bijection onto [0, cells).
// Built and run by tests/test_bp_qcell_cpu.py:
//   g++ -std=c++17 -O1 -g -Wall -Werror -ffp-contract=off -fsanitize=address,undefined -I maskclustering_amd/csrc
//       scripts/bp_qcell_check.cpp -o bp_qcell_check && ./bp_qcell_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "mc_bp_qcell.hpp"

static int bad = 0;
#define CHECK(cond)                                                  \
    do {                                                             \
        if (!(cond)) {                                               \
            if (bad < 20) printf("line %d: %s\n", __LINE__, #cond);  \
            bad++;                                                   \
        }                                                            \
    } while (0)

using namespace mc;

static float next_up(float v) { return std::nextafterf(v, INFINITY); }
static float next_down(float v) { return std::nextafterf(v, -INFINITY); }

// values on and next to cell borders of a grid of width w, near and at the clamps, and plain ones
static std::vector<float> border_values(float w, std::mt19937 &rng)
{
    std::vector<float> v;
    std::uniform_int_distribution<int> cell(-40, 40);
    for (int i = 0; i < 24; i++) {
        const float b = static_cast<float>(cell(rng)) * w;
        v.push_back(b), v.push_back(next_up(b)), v.push_back(next_down(b));
    }
    for (const double edge : {-1.0 * kCellBias, 1.0 * kCellBias - 1.0, 1.0 * kCellBias})  // the clamps
        for (const double off : {-3.0, -1.0, 0.0, 1.0, 3.0, 1000.0, -1000.0}) {
            const float b = static_cast<float>((edge + off) * static_cast<double>(w));
            v.push_back(b), v.push_back(next_up(b)), v.push_back(next_down(b));
        }
    v.push_back(0.0f), v.push_back(-0.0f);
    std::uniform_real_distribution<float> u(-6.0f, 6.0f);
    for (int i = 0; i < 40; i++) v.push_back(u(rng));
    return v;
}

int main()
{
    std::mt19937 rng(12345);
    long long boxes = 0, points = 0, cells_checked = 0;
    for (const float radius : {0.03f, 0.02f, 0.05f, 0.0371f}) {
        const float inv = 1.0f / (2.0f * radius);
        const float w = 2.0f * radius;
        // scene_cell is monotone and stays within the biased range
        {
            std::vector<float> v = border_values(w, rng);
            for (const float a : v)
                for (const float b : v) {
                    const int ca = scene_cell(a, inv), cb = scene_cell(b, inv);
                    CHECK(ca >= 0 && ca < 2 * kCellBias);
                    if (a <= b) CHECK(ca <= cb);
                }
        }
        // box ranges hold every strictly inside point, per axis and as a cell of the box
        for (int rep = 0; rep < 60; rep++) {
            const std::vector<float> v = border_values(w, rng);
            std::uniform_int_distribution<size_t> pick(0, v.size() - 1);
            float lo[3], hi[3];
            for (int a = 0; a < 3; a++) {
                float x = v[pick(rng)], y = v[pick(rng)];
                // three axes near the clamps would give boxes of 2^60 cells: keep two axes local
                if (a > 0) x = std::fmod(x, 8.0f), y = std::fmod(y, 8.0f);
                lo[a] = std::fmin(x, y), hi[a] = std::fmax(x, y);
            }
            const QcBox bx = qc_box(lo, hi, inv);
            boxes++;
            for (int a = 0; a < 3; a++) CHECK(bx.n[a] >= 1 && bx.o[a] >= 0 && bx.o[a] + bx.n[a] <= 2 * kCellBias);
            const int cap = 4096;
            const long long nc = qc_cells_capped(bx, cap);
            const double exact = static_cast<double>(bx.n[0]) * bx.n[1] * bx.n[2];
            CHECK(exact <= cap ? nc == static_cast<long long>(exact) : nc == cap + 1);
            CHECK(qc_cells_capped(bx, 0) == 1);  // a cap of 0 stages nothing
            for (int k = 0; k < 400; k++) {
                float p[3];
                bool inside = true;
                for (int a = 0; a < 3; a++) {
                    // border values, the box's own corners and their float neighbours, and points between
                    const int how = static_cast<int>(rng() % 6);
                    p[a] = how == 0 ? v[pick(rng)] : how == 1 ? next_up(lo[a]) : how == 2 ? next_down(hi[a])
                         : how == 3 ? lo[a] : how == 4 ? hi[a]
                         : lo[a] + (hi[a] - lo[a]) * std::generate_canonical<float, 24>(rng);
                    inside = inside && p[a] > lo[a] && p[a] < hi[a];  // the crop's strict predicate
                }
                if (!inside) continue;
                points++;
                int c[3];
                for (int a = 0; a < 3; a++) {
                    c[a] = scene_cell(p[a], inv);
                    CHECK(c[a] >= bx.o[a] && c[a] < bx.o[a] + bx.n[a]);
                }
                if (nc <= cap) {
                    const int d = qc_local(qc_key(c[0], c[1], c[2]), bx);
                    CHECK(d >= 0 && d < nc);
                }
            }
            // the numbering is a bijection onto [0, cells)
            if (nc <= cap) {
                std::vector<char> seen(static_cast<size_t>(nc), 0);
                for (int z = 0; z < bx.n[2]; z++)
                    for (int y = 0; y < bx.n[1]; y++)
                        for (int x = 0; x < bx.n[0]; x++) {
                            const unsigned long long key = qc_key(bx.o[0] + x, bx.o[1] + y, bx.o[2] + z);
                            const int d = qc_local(key, bx);
                            CHECK(d >= 0 && d < nc);
                            if (d < 0 || d >= nc) continue;
                            CHECK(!seen[d]);
                            seen[d] = 1;
                            int cx, cy, cz;
                            qc_cell_of(d, bx, cx, cy, cz);
                            CHECK(qc_key(cx, cy, cz) == key);
                            if (x + 1 < bx.n[0]) CHECK(qc_local(qc_key(bx.o[0] + x + 1, bx.o[1] + y, bx.o[2] + z), bx) == d + 1);
                            cells_checked++;
                        }
                for (const char s : seen) CHECK(s);
            }
        }
    }
    // a box over the whole clamped range: counted without overflow
    {
        const float lo[3] = {-1e6f, -1e6f, -1e6f}, hi[3] = {1e6f, 1e6f, 1e6f};
        const QcBox bx = qc_box(lo, hi, 1.0f / 0.06f);
        CHECK(bx.n[0] == 2 * kCellBias && bx.o[0] == 0);
        CHECK(qc_cells_capped(bx, 4096) == 4097);
        CHECK(qc_cells_capped(bx, 2147483647) == 2147483648ll);
    }
    printf("boxes=%lld inside_points=%lld cells=%lld bad=%d\n", boxes, points, cells_checked, bad);
    return bad ? 1 : (points > 1000 && cells_checked > 1000 ? 0 : 2);
}
