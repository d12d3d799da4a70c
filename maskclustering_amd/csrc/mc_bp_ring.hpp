// mc_bp_ring.hpp — S1 denoise: the ring search of the deferred points (k_bp_knn_ring, mc_bp_denoise.inl) over
// a slot's hashed grid.  Plain C++17 without a HIP include, usable from host and device;
// scripts/bp_ring_check.cpp checks it on the CPU (tests/test_bp_ring_cpu.py).
//  * A point searches two rings of cells around its own: ring 0, the 27 cells of the 3 x 3 x 3 cube (its own
//    cell first), and ring 1, the 98 cells of the 5 x 5 x 5 cube's shell.  ring_cell(ring, i) is the offset
//    of cell i; over i in [0, ring_cells(ring)) every cell of the ring comes exactly once.
//  * ring_gap is the distance along one axis from the point (at offset o in [0, ce] in its cell) to a cell d
//    cells away, shrunk by sl (1e-9 ce) so that the bound stays below every point's computed distance;
//    ring_gap2 is the squared gap of a cell, ring_culled the test against the current k-th distance: a
//    culled cell holds no point nearer than that, so leaving it out changes none of the k smallest.
//  * RingMask is a lane's set of cells to walk (98 bits), in two words with static names.
//  * ring_mark and ring_walk are the search of one ring, a lane (thread) per point.  ring_mark tests every
//    cell of the ring against the point's own k-th distance and reads the two bucket bounds of the cells it
//    keeps, kRingMarkGroup cells' loads issued before the first is used (they are independent: one memory
//    round trip per group, not one per cell), and marks the cells whose bucket holds records.  ring_walk goes
//    through the records of the marked cells' buckets in one loop, two records per trip; it takes its next
//    cell in the trip that finishes the last one, re-tests it against the k-th distance as it stands then,
//    and reads the bounds of the cell after that, so those are in flight while this cell's records are
//    scanned.  Buckets are shared between cells: the key test per record separates them.
//    The grid is a template parameter: bucket(x, y, z), start(b) (records of bucket b: [start(b),
//    start(b + 1))), rec(q) (a record with x, y, z), key(rec) and cell_key(x, y, z) (what key(rec) is for a
//    record of that cell that counts).
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MC_RING_HD __host__ __device__ __forceinline__
#define MC_RING_UNROLL _Pragma("unroll")
#define MC_RING_ROLLED _Pragma("unroll 1")
#else
#define MC_RING_HD inline
#define MC_RING_UNROLL
#define MC_RING_ROLLED
#endif

namespace mc {

constexpr int kRingInner = 27;      // cells of ring 0: the 3 x 3 x 3 cube
constexpr int kRingShell = 98;      // cells of ring 1: the shell of the 5 x 5 x 5 cube
constexpr int kRingMarkGroup = 8;   // cells whose bucket bounds ring_mark reads together

MC_RING_HD int ring_cells(int ring) { return ring == 0 ? kRingInner : kRingShell; }

// the offset of cell i of a ring
MC_RING_HD void ring_cell(int ring, int i, int &dx, int &dy, int &dz)
{
    if (ring == 0) {  // the own cell (13 of the cube, x fastest), then the other 26 in the cube's order
        const int d = i == 0 ? 13 : (i <= 13 ? i - 1 : i);
        dx = d % 3 - 1;
        dy = (d / 3) % 3 - 1;
        dz = d / 9 - 1;
    } else if (i < 50) {  // the faces z = -2 and z = 2, 5 x 5 cells each
        const int j = i < 25 ? i : i - 25;
        dx = j % 5 - 2;
        dy = j / 5 - 2;
        dz = i < 25 ? -2 : 2;
    } else {  // z = -1, 0, 1: the 16 cells of the 5 x 5 frame (rows y = -2 and y = 2, then the two columns)
        const int j = i - 50, p = j % 16;
        dz = j / 16 - 1;
        if (p < 10) {
            dx = p % 5 - 2;
            dy = p < 5 ? -2 : 2;
        } else {
            dx = (p & 1) ? 2 : -2;
            dy = (p - 10) / 2 - 1;
        }
    }
}

// the gap along one axis to a cell d cells away, from offset o in the own cell of width ce
MC_RING_HD double ring_gap(int d, double o, double ce, double sl)
{
    if (d == 0) return 0.0;
    const double g = (d > 0 ? d * ce - o : -d * ce - (ce - o)) - sl;
    return g > 0.0 ? g : 0.0;
}

MC_RING_HD double ring_gap2(int dx, int dy, int dz, double ox, double oy, double oz, double ce, double sl)
{
    const double gx = ring_gap(dx, ox, ce, sl), gy = ring_gap(dy, oy, ce, sl), gz = ring_gap(dz, oz, ce, sl);
    return (gy * gy + gz * gz) + gx * gx;
}

// a cell whose squared gap reaches the current k-th squared distance holds nothing that enters the list
MC_RING_HD bool ring_culled(double gap2, double kth) { return gap2 >= kth; }

struct RingMask {
    unsigned long long lo = 0, hi = 0;  // bit i % 64 of word i / 64: cell i of the ring

    MC_RING_HD void set(int i, bool on)
    {
        const unsigned long long b = on ? 1ull : 0ull;
        if (i < 64) lo |= b << i;
        else hi |= b << (i - 64);
    }
    MC_RING_HD bool test(int i) const { return ((i < 64 ? lo >> i : hi >> (i - 64)) & 1ull) != 0; }
    MC_RING_HD bool any() const { return (lo | hi) != 0; }
    // the lowest marked cell, removed (any() holds)
    MC_RING_HD int pop()
    {
        int n = 0;
        unsigned long long w = lo;
        if (lo) {
            lo &= lo - 1;
        } else {
            w = hi;
            hi &= hi - 1;
            n = 64;
        }
        return n + __builtin_ctzll(w);
    }
};

// the searching point's place in its grid, as ring_mark and ring_walk take it (any type with these members; the
// kernel's keeps the values in LDS, read where they are used, so that they hold no registers during the walk)
struct RingWhere {
    int c[3];     // its cell
    double o[3];  // its offsets in the cell, each in [0, ce]
    MC_RING_HD int x() const { return c[0]; }
    MC_RING_HD int y() const { return c[1]; }
    MC_RING_HD int z() const { return c[2]; }
    MC_RING_HD double ox() const { return o[0]; }
    MC_RING_HD double oy() const { return o[1]; }
    MC_RING_HD double oz() const { return o[2]; }
};

// the cells of a ring that the point at w must walk: not culled against kth, bucket not empty
template <typename Grid, typename Where>
MC_RING_HD RingMask ring_mark(const Grid &g, int ring, const Where &w, double ce, double sl, double kth)
{
    RingMask m;
    const int nc = ring_cells(ring);
    const int x = w.x(), y = w.y(), z = w.z();
    const double ox = w.ox(), oy = w.oy(), oz = w.oz();
    MC_RING_ROLLED
    for (int i0 = 0; i0 < nc; i0 += kRingMarkGroup) {
        int s[kRingMarkGroup], e[kRingMarkGroup];
        unsigned keep = 0;
        MC_RING_UNROLL
        for (int u = 0; u < kRingMarkGroup; u++) {
            int dx, dy, dz;
            ring_cell(ring, i0 + u < nc ? i0 + u : 0, dx, dy, dz);
            const bool k = i0 + u < nc && !ring_culled(ring_gap2(dx, dy, dz, ox, oy, oz, ce, sl), kth);
            // (a culled cell reads bucket 0, so that the loads stay unconditional and go out together)
            const unsigned b = k ? g.bucket(x + dx, y + dy, z + dz) : 0u;
            s[u] = g.start(b);
            e[u] = g.start(b + 1u);
            keep |= (k ? 1u : 0u) << u;
        }
        MC_RING_UNROLL
        for (int u = 0; u < kRingMarkGroup; u++) m.set(i0 + u, ((keep >> u) & 1u) != 0 && e[u] > s[u]);
    }
    return m;
}

// the records of the marked cells: take(d2, on) for every record, on = its key is its cell's (the others are
// not to be counted: buckets are shared), d2 the squared distance from (ax, ay, az) as ((dx dx + dy dy) + dz dz);
// kth() is the current k-th squared distance
template <typename Grid, typename Where, typename Kth, typename Take>
MC_RING_HD void ring_walk(const Grid &g, int ring, RingMask m, const Where &w, double ax, double ay, double az, double ce,
                          double sl, Kth &&kth, Take &&take)
{
    // the next marked cell: its bucket range ({0, 0}: none left) and its offsets, packed (three bits each,
    // biased by 2: one register from here to the trip that takes the cell, where its key and gap are made)
    auto next = [&](int &s, int &e, int &off) {
        s = e = 0;
        if (!m.any()) return;
        int dx, dy, dz;
        ring_cell(ring, m.pop(), dx, dy, dz);
        off = (dx + 2) | ((dy + 2) << 3) | ((dz + 2) << 6);
        const unsigned b = g.bucket(w.x() + dx, w.y() + dy, w.z() + dz);
        s = g.start(b);
        e = g.start(b + 1u);
    };
    auto visit = [&](const auto &p, unsigned long long key) {
        const double ex = ax - p.x, ey = ay - p.y, ez = az - p.z;
        take(((ex * ex) + (ey * ey)) + (ez * ez), g.key(p) == key);
    };
    unsigned long long key = 0;
    int ns, ne, noff = 0, q = 0, e = 0;
    next(ns, ne, noff);
    MC_RING_ROLLED
    while (true) {
        if (q >= e) {
            if (ns >= ne) break;  // (only cells with records are marked)
            const int dx = (noff & 7) - 2, dy = ((noff >> 3) & 7) - 2, dz = (noff >> 6) - 2;
            // (a cell culled by now keeps one trip, in which no key matches: ~0 is a key no record has)
            const bool cull = ring_culled(ring_gap2(dx, dy, dz, w.ox(), w.oy(), w.oz(), ce, sl), kth());
            key = cull ? ~0ull : g.cell_key(w.x() + dx, w.y() + dy, w.z() + dz);
            q = ns;
            e = cull ? ns + 1 : ne;
            next(ns, ne, noff);
        }
        const auto p0 = g.rec(q), p1 = g.rec(q + 1 < e ? q + 1 : q);
        visit(p0, key);
        visit(p1, q + 1 < e ? key : ~0ull);
        q += 2;
    }
}

}  // namespace mc
