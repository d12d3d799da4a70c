// mc_bp_denoise_lds.inl — S1 back-projection, bp_launch_denoise: the size classes, k_bp_classify and
// the LDS-resident kernel of each class, with the eps-list helpers and cell walks it is built from.
namespace mc {

// Size classes of the LDS-resident kernel: capacity N points, T threads, and the workgroups per CU
// the LDS footprint (72 B per point) admits.  Slots of more than kBpLdsN voxels take k_bp_denoise.
constexpr int kBpLdsN = 16384;  // largest class of the LDS-kernel template
constexpr int kBpClasses = 6;   // the classes of kBpClassN; class kBpClasses = k_bp_denoise
constexpr int kBpStreamClasses = 5;  // classes with a stream of their own (the 16384 class shares the side stream)
// The classes' capacities, ascending (class index = position): the one list that k_bp_classify's
// thresholds and the host's launches and per-class regions (mc_bp_host.inl) read.
constexpr int kBpClassN[] = {512, 1024, 2048, 3072, 4096, 16384};
static_assert(sizeof(kBpClassN) / sizeof(kBpClassN[0]) == kBpClasses && kBpClasses == kBpStreamClasses + 1,
              "one entry per LDS class; every class but the last has a stream of its own");
static_assert(kBpClassN[kBpClasses - 1] == kBpLdsN, "the last class is the LDS kernel's largest");
constexpr int kBpNbCap = 64;  // eps-neighbour list entries per point (self included); more -> cell walk
constexpr int kBpKnnBatch = 4;  // k-NN list pass: selected entries fetched per batch
template <int N>
struct BpLdsClass;
#ifndef MC_BP_WG512
#define MC_BP_WG512 4  // workgroups per CU the 512 class is compiled for (register budget)
#endif
#ifndef MC_BP_WG1024
#define MC_BP_WG1024 2
#endif
// kLean: 0 = everything in LDS; 1 = one bucket per point, sort/rank/label/statistics arrays in global
// scratch; 2 = also the neighbour counts and the union-find array in global scratch
template <>
struct BpLdsClass<512> {
    static constexpr int T = 256, kWgPerCu = MC_BP_WG512, kLean = 0;
};
template <>
struct BpLdsClass<1024> {
    static constexpr int T = 512, kWgPerCu = MC_BP_WG1024, kLean = 0;
};
#ifndef MC_BP_TBIG
#define MC_BP_TBIG 1024  // threads of the one-workgroup-per-CU classes (2048, 3072, 4096)
#endif
template <>
struct BpLdsClass<2048> {
    static constexpr int T = MC_BP_TBIG, kWgPerCu = 1, kLean = 0;
};
template <>
struct BpLdsClass<3072> {
    static constexpr int T = MC_BP_TBIG, kWgPerCu = 1, kLean = 1;
};
template <>
struct BpLdsClass<4096> {
    static constexpr int T = MC_BP_TBIG, kWgPerCu = 1, kLean = 2;
};
template <>  // kLean 3: every per-point array in global scratch (large, rare slots)
struct BpLdsClass<16384> {
    static constexpr int T = 1024, kWgPerCu = 1, kLean = 3;
};
template <int N>
constexpr bool kBpLean = BpLdsClass<N>::kLean >= 1;
template <int N>
constexpr bool kBpLean2 = BpLdsClass<N>::kLean >= 2;
template <int N>
constexpr bool kBpLean3 = BpLdsClass<N>::kLean >= 3;
// global scratch ints per workgroup of a lean class: [lean 3: cell-sorted points (8N), bucket starts
// (N + 1, padded to N + 8)] savg (2N), sB (2N + 2), sX (N), sorig + spos (N) [lean 2: + sflag (N),
// spar (N)]; a multiple of 8 ints, so every region stays 32-byte aligned
template <int N>
constexpr size_t kBpLean3Pre = kBpLean3<N> ? 9 * static_cast<size_t>(N) + 8 : 0;
template <int N>
constexpr size_t kBpLeanInts =
    kBpLean<N> ? ((kBpLean3Pre<N> + (kBpLean2<N> ? 8 : 6) * static_cast<size_t>(N) + 2 + 7) / 8) * 8 : 0;

struct BpLdsGrid {
    const double4 *pt;  // x, y, z, cell key bits (bit 63: kept by the class filter) per sorted position
    const int *bs;      // bucket starts (2n + 1)
    unsigned nb;
    int cmax[3];
};

constexpr unsigned long long kKeptBit = 1ull << 63;
constexpr int kBpCellMax = (1 << 21) - 2;  // denoise grid cells per axis: pack3's 21 bits, a neighbour's + 1 included
constexpr int kLdsCellUnroll = 2;  // records in flight per cell scan (VGPR budget: 128 at 4 waves/SIMD)

// fn(q, d2) for every sorted position q of cell (x, y, z) whose key (with `with` bits set) matches;
// d2 = squared distance from a (u3 order).  Records are read kLdsCellUnroll at a time so their LDS loads overlap.
template <typename Fn>
__device__ __forceinline__ void lds_cell(const BpLdsGrid &g, int x, int y, int z, unsigned long long with, double ax,
                                         double ay, double az, Fn &&fn)
{
    // (no bounds test: coordinates are >= -2 (the origin lies below every point) and far below
    // kBpCellMax; a negative one makes a key with its top bits set, which no record has)
    const unsigned long long key = pack3(x, y, z) | with;
    const unsigned long long mask = ~0ull ^ (with ? 0ull : kKeptBit);
    const unsigned b = mod_mul(bp_hash3(x, y, z), g.nb);
    const int e = g.bs[b + 1];
    int q = g.bs[b];
    for (; q + kLdsCellUnroll <= e; q += kLdsCellUnroll) {
        double4 p[kLdsCellUnroll];
#pragma unroll
        for (int u = 0; u < kLdsCellUnroll; u++) p[u] = g.pt[q + u];
#pragma unroll
        for (int u = 0; u < kLdsCellUnroll; u++) {
            if ((static_cast<unsigned long long>(__double_as_longlong(p[u].w)) & mask) != key) continue;
            const double dx = ax - p[u].x, dy = ay - p[u].y, dz = az - p[u].z;
            fn(q + u, ((dx * dx) + (dy * dy)) + (dz * dz));
        }
    }
    for (; q < e; q++) {
        const double4 p = g.pt[q];
        if ((static_cast<unsigned long long>(__double_as_longlong(p.w)) & mask) != key) continue;
        const double dx = ax - p.x, dy = ay - p.y, dz = az - p.z;
        fn(q, ((dx * dx) + (dy * dy)) + (dz * dz));
    }
}

// the 27 cells around (x, y, z); the next cell's bucket range is read from LDS while this cell's
// records are scanned (one dependent LDS round trip less per cell)
template <typename Fn>
__device__ __forceinline__ void lds_cells27(const BpLdsGrid &g, int x, int y, int z, unsigned long long with, double ax,
                                            double ay, double az, Fn &&fn)
{
    const unsigned long long mask = ~0ull ^ (with ? 0ull : kKeptBit);
    auto range = [&](int d, unsigned long long &key) {
        const int cx = x + d % 3 - 1, cy = y + (d / 3) % 3 - 1, cz = z + d / 9 - 1;
        // (no bounds test: coordinates are >= -2 (the origin lies below every point) and far below
        // kBpCellMax; a negative one makes a key with its top bits set, which no record has)
        key = pack3(cx, cy, cz) | with;
        const unsigned b = mod_mul(bp_hash3(cx, cy, cz), g.nb);
        return make_int2(g.bs[b], g.bs[b + 1]);
    };
    unsigned long long nkey = 0;
    int2 nr = range(0, nkey);
#pragma unroll 1
    for (int d = 0; d < 27; d++) {  // rolled: one copy of fn (instruction cache)
        const unsigned long long key = nkey;
        const int2 r = nr;
        if (d + 1 < 27) nr = range(d + 1, nkey);
        int q = r.x;
        const int e = r.y;
        for (; q + kLdsCellUnroll <= e; q += kLdsCellUnroll) {
            double4 p[kLdsCellUnroll];
#pragma unroll
            for (int u = 0; u < kLdsCellUnroll; u++) p[u] = g.pt[q + u];
#pragma unroll
            for (int u = 0; u < kLdsCellUnroll; u++) {
                if ((static_cast<unsigned long long>(__double_as_longlong(p[u].w)) & mask) != key) continue;
                const double dx = ax - p[u].x, dy = ay - p[u].y, dz = az - p[u].z;
                fn(q + u, ((dx * dx) + (dy * dy)) + (dz * dz));
            }
        }
        for (; q < e; q++) {
            const double4 p = g.pt[q];
            if ((static_cast<unsigned long long>(__double_as_longlong(p.w)) & mask) != key) continue;
            const double dx = ax - p.x, dy = ay - p.y, dz = az - p.z;
            fn(q, ((dx * dx) + (dy * dy)) + (dz * dz));
        }
    }
}

// Per-workgroup eps-neighbour lists: slot k of sorted position q is the u16 at uint4 index
// (k / 8) * N + q, half-word k % 8: a wave's stores of one k fall on 16-byte strided words (few cache
// lines), and a point's whole list (<= 64 slots) is 8 uint4 loads issued before the first is used.
// An entry is the neighbour's sorted position and, in the bits above it, its k-NN distance class; the
// k-NN's candidate selection reads the classes instead of recomputing distances.  Two formats by N:
//  * N <= 4096: 12 bits of position and four of class, one of 16 classes of equal width in d2
//    (mc::knn_class, mc_bp_knnsel.hpp);
//  * N = 16384: 14 bits of position and two of class: 0 / 1 / 2 = inside knn_r2[0 / 1 / 2] (0.6 / 0.75 /
//    0.9 eps), 3 = the rest of the eps ball.
// kNbPos<N> / kNbShift<N> decode an entry at every site that reads one (union, border labels, k-NN).
// sflag[q] = count (bits 0-14, self included) | kept (bit 30).
// (Measured and not kept: the near entries in a prefix region of their own, so that the k-NN of a
// point with >= k near entries reads them with static register indices: C3 denoise +4 %, C2 +5 %.)
template <int N>
constexpr bool kNbFine = N <= 4096;  // the 16-class entry format and the one-round k-NN list pass
template <int N>
constexpr unsigned kNbShift = kNbFine<N> ? 12u : 14u;
template <int N>
constexpr unsigned kNbPos = (1u << kNbShift<N>) - 1u;
constexpr int kNbCnt = 0x7FFF;
static_assert(kBpLdsN <= 16384, "sorted positions fit 14 bits, counts 15 bits");
__device__ __forceinline__ int nb_cnt(int f) { return f & kNbCnt; }
template <int N>
__device__ __forceinline__ void nb_put(unsigned short *__restrict__ nbw, int q, int k, unsigned e)
{
    // 32-bit offset (< 8 * 64 * N <= 2^23): a store with the workgroup's region base in SGPRs and one
    // VGPR offset, no 64-bit address arithmetic per store
    const unsigned off = ((static_cast<unsigned>(k) >> 3) * static_cast<unsigned>(N) + static_cast<unsigned>(q)) * 8u +
                         (static_cast<unsigned>(k) & 7u);
    *reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(nbw) + (off << 1)) = static_cast<unsigned short>(e);
}
template <int N>
__device__ __forceinline__ unsigned nb_class(double d2, const BpDev &pr)
{
    if constexpr (kNbFine<N>) return mc::knn_class(d2, pr.knn_s);
    else return 3u - (d2 < pr.knn_r2[0] ? 1u : 0u) - (d2 < pr.knn_r2[1] ? 1u : 0u) - (d2 < pr.knn_r2[2] ? 1u : 0u);
}
// the union's sampled far links (step 6) by class: farA takes the outer part of the eps ball (d >= 0.9 eps:
// class 3 of the 2-bit format, classes 13 .. 15 of the 16), farB the ring inside it (0.75 .. 0.9 eps:
// class 2, classes 9 .. 12)
template <int N>
__device__ __forceinline__ bool nb_far_a(unsigned c) { return kNbFine<N> ? c >= 13u : c == 3u; }
template <int N>
__device__ __forceinline__ bool nb_far_b(unsigned c) { return kNbFine<N> ? c - 9u <= 3u : c == 2u; }

// The list builders' walk over the records of ranges d0 .. 26 (range(d, key): the bucket range of
// cell d and its key), flat: a lane goes through the records of its non-empty ranges in one loop,
// two per trip, and takes its next range in the trip that finishes the last one (that range was read
// while the last one's records were scanned).  A wave holds points of several cells (consecutive
// positions of the hash order) whose neighbourhoods are filled differently: a loop per cell runs
// every cell for the lane with the most records in that cell, the flat loop for the lane with the
// most records in all (C3 and C2 denoise -3 %, docs/experiments.md "own-walk lists").
// visit(record, position, key) tests one record; the key ~0, which no record has, masks the second
// record of a trip past the range's end.
template <typename Range, typename Visit>
__device__ __forceinline__ void lds_flat_walk(const BpLdsGrid &g, int d0, Range &&range, Visit &&visit)
{
    unsigned cells = 0;  // bit d: range d holds records
#pragma unroll 3
    for (int d = d0; d < 27; d++) {
        unsigned long long k;
        const int2 r = range(d, k);
        cells |= (r.y > r.x ? 1u : 0u) << d;
    }
    auto next = [&](unsigned long long &k) {  // the next non-empty range ({0, 0}: none left)
        if (!cells) return make_int2(0, 0);
        const int d = __ffs(static_cast<int>(cells)) - 1;
        cells &= cells - 1;
        return range(d, k);
    };
    unsigned long long key = 0, nkey = 0;
    int2 nr = next(nkey);
    int q2 = 0, e = 0;
#pragma unroll 1
    while (true) {
        if (q2 >= e) {
            if (nr.x >= nr.y) break;
            key = nkey;
            q2 = nr.x;
            e = nr.y;
            nr = next(nkey);
        }
        const double4 p0 = g.pt[q2], p1 = g.pt[min(q2 + 1, e - 1)];
        visit(p0, q2, key);
        visit(p1, q2 + 1, q2 + 1 < e ? key : ~0ull);
        q2 += 2;
    }
}

// The eps-neighbour list of sorted position q (point a, cell (x, y, z)), built by the lane that owns
// q (the classes whose counts live in global scratch): every point of the 27 cells with d2 < eps2
// (self included), in cell-walk order.  One predicate per candidate (cell key and distance together,
// the record loaded whole).  The entries are packed in registers (mc::NbPack, mc_bp_nbpack.hpp) and
// leave as whole 16-byte words: one store per eight entries, and the last, partial word after the
// walk with its unused half-words zero.  Entries past kBpNbCap are counted and not stored (the list
// is unused then: the point walks its cells).  farA / farB: the last neighbour of the two outer distance
// ranges (nb_far_a / nb_far_b: the union's sampled links, step 6).  Returns the count.
// (Measured and not kept, docs/experiments.md "own-walk lists": this builder in the 512 .. 3072
// classes instead of the pair pass: C3 denoise +15 %, C2 +11 %; it tests twice the candidates, and
// the pair pass's LDS atomics and 2-byte stores cost less than those tests.)
template <int N>
__device__ __forceinline__ int lds_eps_own(const BpLdsGrid &g, int x, int y, int z, double ax, double ay, double az,
                                           const BpDev &pr, unsigned short *__restrict__ nbw, int q, int &farA,
                                           int &farB)
{
    auto range = [&](int d, unsigned long long &key) {
        const int cx = x + d % 3 - 1, cy = y + (d / 3) % 3 - 1, cz = z + d / 9 - 1;
        // (no bounds test: coordinates are >= -2 (the origin lies below every point) and far below
        // kBpCellMax; a negative one makes a key with its top bits set, which no record has)
        key = pack3(cx, cy, cz);
        const unsigned b = mod_mul(bp_hash3(cx, cy, cz), g.nb);
        return make_int2(g.bs[b], g.bs[b + 1]);
    };
    // word u of q's list: byte (u * N + q) * 16 of the region (a 32-bit offset, < 128 * N <= 2^21: a
    // store with the workgroup's region base in SGPRs and one VGPR offset, no 64-bit address arithmetic)
    auto put = [&](const mc::NbPack &acc, int cnt) {
        const unsigned off =
            (static_cast<unsigned>(mc::nb_store_word(cnt)) * static_cast<unsigned>(N) + static_cast<unsigned>(q)) * 16u;
        *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(nbw) + off) = make_uint4(acc.a0, acc.a1, acc.a2, acc.a3);
    };
    const double eps2 = pr.eps2;
    int cnt = 0;
    int fa = farA, fb = farB;  // locals, selected: written through the references they live in scratch
    mc::NbPack acc;
    auto visit = [&](const double4 &p, int q2, unsigned long long key) {
        const double dx = ax - p.x, dy = ay - p.y, dz = az - p.z;
        const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        if (static_cast<unsigned long long>(__double_as_longlong(p.w)) == key && d2 < eps2) {  // (no kept bits yet)
            const unsigned c = nb_class<N>(d2, pr);
            acc.push(static_cast<unsigned>(q2) | (c << kNbShift<N>));
            fa = nb_far_a<N>(c) ? q2 : fa;
            fb = nb_far_b<N>(c) ? q2 : fb;
            cnt++;
            if (mc::nb_store_full(cnt, kBpNbCap)) put(acc, cnt);
        }
    };
    lds_flat_walk(g, 0, range, visit);
    if (mc::nb_store_tail(cnt, kBpNbCap)) {
        acc.flush(cnt & (mc::kNbWordSlots - 1));
        put(acc, cnt);
    }
    farA = fa;
    farB = fb;
    return cnt;
}

// The same lists built from each unordered pair once (classes whose counts live in LDS): sorted
// position q visits half of its own bucket cyclically and the 13 cells after its own in (z, y, x)
// order; a pair within eps is appended to both lists, each at the slot an LDS atomic on its counter
// returns (sflag[] holds the counts, self entries already in slot 0).  Half the candidate records of
// lds_eps_own; the slot order within a list is arbitrary, which no consumer depends on (the union
// and the border labels are order-free, the k-NN sorts).  Own bucket [s, e) of c positions: q
// visits the next h positions cyclically, h = (c - 1) / 2, plus the opposite one when c is even and
// q is in the first half, so every pair of the bucket is visited once and each point's first list
// entries (the union's first sampled link, step 6) mix earlier and later positions of its cell.
template <int N>
__device__ __forceinline__ void lds_eps_pairs(const BpLdsGrid &g, int x, int y, int z, double ax, double ay, double az,
                                              const BpDev &pr, unsigned short *__restrict__ nbw, int q, int *sflag,
                                              int *farA, int *farB)
{
    const unsigned b0 = mod_mul(bp_hash3(x, y, z), g.nb);
    const int s0 = g.bs[b0], e0 = g.bs[b0 + 1], c0 = e0 - s0;
    const int h0 = (c0 - 1) / 2 + ((c0 % 2 == 0 && q - s0 < c0 / 2) ? 1 : 0);
    const int f1 = min(q + 1 + h0, e0);               // forward part [q + 1, f1)
    const int w1 = s0 + max(0, q + 1 + h0 - e0);      // wrapped part [s0, w1)
    auto range = [&](int d, unsigned long long &key) {
        if (d <= 13) {  // 12: the own bucket's wrapped part, 13: its forward part
            key = pack3(x, y, z);
            return d == 12 ? make_int2(s0, w1) : make_int2(q + 1, f1);
        }
        const int cx = x + d % 3 - 1, cy = y + (d / 3) % 3 - 1, cz = z + d / 9 - 1;
        // (no bounds test: coordinates are >= -2 (the origin lies below every point) and far below
        // kBpCellMax; a negative one makes a key with its top bits set, which no record has)
        key = pack3(cx, cy, cz);
        const unsigned b = mod_mul(bp_hash3(cx, cy, cz), g.nb);
        return make_int2(g.bs[b], g.bs[b + 1]);
    };
    const double eps2 = pr.eps2;
    int fa = q, fb = q;
    auto visit = [&](const double4 &p, int q2, unsigned long long key) {
        const double dx = ax - p.x, dy = ay - p.y, dz = az - p.z;
        const double d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        // (no record carries the kept bit yet: the class filter sets it after the lists are built)
        if (static_cast<unsigned long long>(__double_as_longlong(p.w)) == key && d2 < eps2) {
            // both slots' atomics in flight together; the distance class and the far links (the two outer
            // distance ranges of this point's forward walk: the union's sampled links, step 6, stored
            // once after the walk) computed under them; one wait before the stores.  Entries past
            // the cap overwrite the last slot: every slot still holds a neighbour,
            // and a list past the cap is not read (its point walks the cells), so no branch
            const int o1 = atomicAdd(&sflag[q], 1), o2 = atomicAdd(&sflag[q2], 1);
            const unsigned c0 = nb_class<N>(d2, pr), c = c0 << kNbShift<N>;
            fa = nb_far_a<N>(c0) ? q2 : fa;
            fb = nb_far_b<N>(c0) ? q2 : fb;
            asm volatile("" ::"v"(o1), "v"(o2), "v"(c));
            nb_put<N>(nbw, q, min(o1, kBpNbCap - 1), static_cast<unsigned>(q2) | c);
            nb_put<N>(nbw, q2, min(o2, kBpNbCap - 1), static_cast<unsigned>(q) | c);
        }
    };
    lds_flat_walk(g, 12, range, visit);
    farA[q] = fa;
    farB[q] = fb;
}

// the uint4 words of sorted position q's first cnt slots, all issued together; the others zero.
// The caller must be the lane that owns q in the list phase (q = t + k * T, as every loop over q in
// k_bp_denoise_lds): lds_eps_own's lists are handed over by program order only, so a reader that takes
// q any other way needs a sync_global() after step 5 first.
template <int N>
__device__ __forceinline__ void nb_load(const unsigned short *__restrict__ nbw, int q, int cnt, unsigned (&w)[32])
{
    static_assert(kBpNbCap == 64, "eight uint4 per point");
    const uint4 *row = reinterpret_cast<const uint4 *>(nbw) + q;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (8 * u < cnt) v = row[static_cast<size_t>(u) * N];
        w[4 * u] = v.x;
        w[4 * u + 1] = v.y;
        w[4 * u + 2] = v.z;
        w[4 * u + 3] = v.w;
    }
}
// slot k of the loaded words (k must be wave-uniform: register-relative moves, no scratch)
__device__ __forceinline__ unsigned nb_ent(const unsigned (&w)[32], int k)
{
    return nb_slot(w, k);  // mc_bp_nbpack.hpp
}

// fn(k, entry, pre(entry)) for slots 0 .. cnt - 1; pre(entry of the next slot) is issued before fn
// runs on this one (its loads overlap fn).  The slot index is the same in every active lane (lanes
// only leave), so the loop keeps one copy of fn's code and reads the words with uniform register
// indices (unrolled copies of a 20-step insertion overflow the instruction cache).
template <typename Pre, typename Fn>
__device__ __forceinline__ void nb_walk(const unsigned (&w)[32], int cnt, Pre &&pre, Fn &&fn)
{
    if (cnt <= 0) return;
    auto nx = pre(nb_ent(w, 0));
#pragma unroll 1
    for (int k = 0; k < cnt; k++) {
        const auto cur = nx;
        const unsigned e = nb_ent(w, k);
        if (k + 1 < cnt) nx = pre(nb_ent(w, k + 1));
        fn(k, e, cur);
    }
}

}  // namespace mc

#include "mc_bp_dbg.inl"  // the diagnostics build's checks of the lists and walks above

namespace mc {

// Slots of each size class (unordered: every slot is processed independently); class kBpClasses =
// more than kBpLdsN voxels (the global-memory kernel).  min_cls > 0 sends small slots to a larger
// class (tests: every class gives the same results).  cls_cnt[kBpClasses + 1] must be zero.
__global__ __launch_bounds__(256) void k_bp_classify(const int *__restrict__ dNS, const int *__restrict__ slot_nv,
                                                     const int *__restrict__ order, int cap, int min_cls,
                                                     int *__restrict__ cls_cnt, int *__restrict__ cls_list)
{
    // slots taken in k_bp_vox_order's largest-first order, so each class's list (its ticket order)
    // starts with its largest slots (roughly: the workgroups append concurrently) and the class
    // ends on small ones instead of a lone large one
    const int NS = *dNS;
    for (int i = blockIdx.x * 256 + threadIdx.x; i - static_cast<int>(threadIdx.x) < NS; i += gridDim.x * 256) {
        const bool live = i < NS;
        const int s = live ? order[i] : 0;
        const int n = live ? slot_nv[s] : 0;
        static_assert(kBpClasses == 6, "one link of the chain per class");
        const int c = max(min_cls, n <= kBpClassN[0] ? 0 : n <= kBpClassN[1] ? 1 : n <= kBpClassN[2] ? 2
                                   : n <= kBpClassN[3] ? 3 : n <= kBpClassN[4] ? 4 : n <= kBpClassN[5] ? 5 : kBpClasses);
#pragma unroll
        for (int k = 0; k <= kBpClasses; k++) {
            const unsigned long long b = __ballot(live && c == k);
            if (!b) continue;
            const int leader = __ffsll(static_cast<long long>(b)) - 1;
            int base = 0;
            if (lane_id() == leader) base = atomicAdd(&cls_cnt[k], __popcll(b));
            base = __shfl(base, leader, 64);
            if (live && c == k) cls_list[k * cap + base + __popcll(b & ((1ull << lane_id()) - 1))] = s;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// (a4) denoise, LDS-resident variant for slots of <= N voxels (the bulk): the same steps as
// k_bp_denoise below, with the points cell-sorted into LDS so that every neighbourhood scan reads
// LDS.  Union-find runs over sorted positions; each component is keyed by its smallest original
// index, which numbers the clusters exactly as k_bp_denoise / Open3D do.  The eps-neighbour scan
// records every point's neighbour positions (<= kBpNbCap, in a per-workgroup global list), so the
// union, border-label and k-NN steps visit those instead of walking 27 hashed cells: the 20 nearest
// kept points of a point with >= 20 kept eps-neighbours are among them (every other point is at
// distance >= eps).  Workgroups take slots of their size class from a ticket counter.
// ---------------------------------------------------------------------------------------------

template <int N>
__global__ __launch_bounds__(BpLdsClass<N>::T, BpLdsClass<N>::kWgPerCu * BpLdsClass<N>::T / 256) void k_bp_denoise_lds(
    const int *__restrict__ cls_cnt, const int *__restrict__ cls_list, int *__restrict__ ticket,
    const int *__restrict__ slot_pix, const int *__restrict__ slot_nv, BpDev pr, const double *__restrict__ vpts,
    unsigned short *__restrict__ nbl, int *__restrict__ lean_scr, int *__restrict__ slot_m, double *__restrict__ gavg,
    int *__restrict__ gsx, double4 *__restrict__ grec, int *__restrict__ gbs, int *__restrict__ gitem,
    int *__restrict__ dq, int *__restrict__ dq_cnt, int dq_cap, double *__restrict__ slot_grid, int *__restrict__ err)
{
    constexpr int T = BpLdsClass<N>::T;
    constexpr int NW = T / 64;
    constexpr bool kLean = kBpLean<N>;
    constexpr int NBK = kLean ? 1 : 2;   // hash buckets per point
    constexpr int kFbCount = 2 * N + 1;  // index of the fallback counter in sB
    constexpr int NL = kLean ? 1 : N;    // extent of the arrays a lean class keeps in global scratch
    constexpr bool kLean3 = kBpLean3<N>;
    // a lean class hands its global-scratch arrays between waves at every barrier (sync_global)
    auto bar = []() {
        if constexpr (kLean) sync_global();
        else __syncthreads();
    };
    __shared__ double4 spt_l[kLean3 ? 1 : N];  // cell-sorted points + cell keys
    __shared__ int sA_l[kLean3 ? 1 : NBK * N + 1];  // bucket starts
    __shared__ int sB_l[2 * NL + 2];     // bucket counts; then min original index per root [0, n) +
                                         // class counts [N, ..); then the k-NN fallback list
    __shared__ short sorig_l[NL], spos_l[NL];  // sorted position <-> original index
    constexpr int NL2 = kBpLean2<N> ? 1 : N;
    __shared__ int sflag_l[NL2];         // eps-neighbour count | kept bit 30
    __shared__ int spar_l[NL2];          // union-find over positions, then roots, then kept ranks
    __shared__ int sX_l[NL];             // bucket per point; rank per root; S list
    __shared__ int slab_l[NL];           // labels (the k-NN means go to the slot's range of gavg)
    int *const gs0 = lean_scr + static_cast<size_t>(blockIdx.x) * kBpLeanInts<N>;
    double4 *const spt = kLean3 ? reinterpret_cast<double4 *>(gs0) : spt_l;
    int *const sA = kLean3 ? gs0 + 8 * N : sA_l;
    int *const gs = gs0 + kBpLean3Pre<N>;
    int *const slab = kLean ? gs : slab_l;
    int *const sB = kLean ? gs + 2 * N : sB_l;
    int *const sX = kLean ? gs + 4 * N + 2 : sX_l;
    short *const sorig = kLean ? reinterpret_cast<short *>(gs + 5 * N + 2) : sorig_l;
    short *const spos = kLean ? sorig + N : spos_l;
    int *const sflag = kBpLean2<N> ? gs + 6 * N + 2 : sflag_l;
    int *const spar = kBpLean2<N> ? gs + 7 * N + 2 : spar_l;
    __shared__ double red[6 * NW];
    __shared__ int ws[NW];
    __shared__ int s_slot, s_ndef;
    int *ccnt = sB + N;
    int *sfb = sB;  // kNN fallback list after the class filter (sB is free by then)
    const int cnt_cls = *cls_cnt;
    const int t = threadIdx.x, lane = lane_id(), wv = t >> 6;
    unsigned short *nbw = nbl + static_cast<size_t>(blockIdx.x) * N * kBpNbCap;
    // one array for the list words of every walk (union, labels, k-NN): the compiler keeps a
    // dynamically indexed array in registers only within a per-function budget, so separate arrays
    // per walk would land in scratch
    unsigned w[32];
#ifdef MC_BP_STAMPS
    unsigned long long stamp_prev = __builtin_amdgcn_s_memrealtime();
#endif
    // Ticket loop invariant: thread 0 overwrites s_slot only after every thread has read it.  The
    // barrier after the read gives that directly (the body also ends in a barrier, and every path
    // through it reaches block barriers, but the loop must not depend on the body's structure).
    while (true) {
        if (t == 0) s_slot = atomicAdd(ticket, 1);
        bar();
        const int tk = s_slot;
        bar();
        if (tk >= cnt_cls) break;
        const int s = cls_list[tk];
        const int base = slot_pix[s], n = slot_nv[s];
#ifdef MC_BP_STAMPS
        const unsigned long long slot_t0 = __builtin_amdgcn_s_memrealtime();
        if (t == 0) {
            atomicAdd(&g_bp_stamps[14], 1ull);
            atomicAdd(&g_bp_stamps[15], static_cast<unsigned long long>(n));
        }
#endif
        BP_STAMP(16);
        const double *P = vpts + 3 * static_cast<size_t>(base);
        // 1. grid origin: the voxel kernel's min bound of the slot (slot_grid[0..2], below every
        //    voxel mean), so no bounding-box pass; the grid is this kernel's own search structure (any
        //    origin below the points gives the same neighbour sets), and cells beyond the points are
        //    empty buckets, so the extent bound is just the key range
        double mn[3];
        {
            const double *gm0 = slot_grid + 8 * static_cast<size_t>(s);
#pragma unroll
            for (int c = 0; c < 3; c++) mn[c] = uniform_d(gm0[c]);
        }
        BpLdsGrid g;
        g.pt = spt;
        g.bs = sA;
        g.nb = static_cast<unsigned>(NBK * n);
#pragma unroll
        for (int c = 0; c < 3; c++) g.cmax[c] = kBpCellMax;
        if (t == 0) {  // the grid's extent and size for k_bp_knn_ring (the origin is in place)
            double *gm = slot_grid + 8 * static_cast<size_t>(s);
#pragma unroll
            for (int c = 0; c < 3; c++) gm[3 + c] = static_cast<double>(kBpCellMax);
            gm[6] = static_cast<double>(g.nb);
            gm[7] = static_cast<double>(n);
        }
        BP_STAMP(17);
        // 2. bucket counts
        for (int b = t; b < NBK * n; b += T) sB[b] = 0;
        bar();
        for (int i = t; i < n; i += T) {
            int c3[3];
#pragma unroll
            for (int c = 0; c < 3; c++) c3[c] = static_cast<int>(floor_div(P[3 * i + c] - mn[c], pr.ce));
            const unsigned b = mod_mul(bp_hash3(c3[0], c3[1], c3[2]), g.nb);
            sX[i] = static_cast<int>(b);
            atomicAdd(&sB[b], 1);
        }
        bar();
        BP_STAMP(18);
        // 3. bucket starts
        {
            int carry = 0;
            for (int b0 = 0; b0 < NBK * n; b0 += T) {
                const int b = b0 + t;
                const int v = b < NBK * n ? sB[b] : 0;
                int tot;
                const int ex = block_excl_scan<T>(v, ws, tot);
                if (b < NBK * n) sA[b] = carry + ex;
                carry += tot;
            }
            if (t == 0) sA[NBK * n] = carry;
        }
        bar();
        BP_STAMP(19);
        // 4. counting-sort scatter into LDS (bucket counters return to zero)
        for (int i = t; i < n; i += T) {
            const int b = sX[i];
            const int q = sA[b] + atomicSub(&sB[b], 1) - 1;
            const double x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
            const unsigned long long ck = pack3(static_cast<int>(floor_div(x - mn[0], pr.ce)),
                                                static_cast<int>(floor_div(y - mn[1], pr.ce)),
                                                static_cast<int>(floor_div(z - mn[2], pr.ce)));
            spt[q] = make_double4(x, y, z, __longlong_as_double(static_cast<long long>(ck)));
            sorig[q] = static_cast<short>(i);
            spos[i] = static_cast<short>(q);
        }
        bar();
        auto keyof = [&](int q) { return static_cast<unsigned long long>(__double_as_longlong(spt[q].w)); };
        BP_STAMP(20);
        // 5. eps-neighbour counts (self included) and lists: from each pair once where the counts
        //    live in LDS, by a full 27-cell walk per point where they are global scratch
        if constexpr (!kBpLean2<N>) {
            for (int q = t; q < n; q += T) {
                sflag[q] = 1;
                nb_put<N>(nbw, q, 0, static_cast<unsigned>(q));  // self, class 0
                spar[q] = q;
            }
            bar();
            for (int q = t; q < n; q += T) {
                int x, y, z;
                unpack3(keyof(q), x, y, z);
                lds_eps_pairs<N>(g, x, y, z, spt[q].x, spt[q].y, spt[q].z, pr, nbw, q, sflag, sX, slab);
            }
            sync_global();  // the lists hold other waves' stores
        } else {
            // (hand-off: the list of q is stored only by the lane that owns q, q = t + k * T, and
            // every reader takes q from a loop of the same shape (the sampled links and the union of
            // step 6, the labels of step 8, the k-NN list pass of step 10, the diagnostics' list
            // check), so a list is read by the lane that stored it, in program order; the counts and
            // far links are read by other lanes after the barrier below, a sync_global() here)
            for (int q = t; q < n; q += T) {
                int x, y, z;
                unpack3(keyof(q), x, y, z);
                const double ax = spt[q].x, ay = spt[q].y, az = spt[q].z;
                int fa = q, fb = q;
                sflag[q] = lds_eps_own<N>(g, x, y, z, ax, ay, az, pr, nbw, q, fa, fb);
                spar[q] = q;
                sX[q] = fa;
                slab[q] = fb;
            }
        }
        bar();
        BP_STAMP(21);
        if constexpr (MC_DBG_CHECK) bp_dbg_lists<N>(g, sflag, nbw, n, pr, s);
        // 6. connected core points, Afforest-style (Sutton et al., SC'18): (a) every core point links to
        //    three sampled core neighbours: its first list entry and two far ones of its own list walk
        //    (radius classes 3 and 2, kept in sX / slab, free between the scatter and the labels: links
        //    that span the eps ball percolate where the nearest few stay in clumps; sampling the first
        //    two entries left most points outside the giant, 63 us per C3 slot against 12);
        //    (b) the component most of a sample of core points
        //    fell into (a slot is mostly one surface patch: ~98 % of its points) is taken as the giant;
        //    (c) only core points outside it unite with all their core neighbours (list, or the 27 cells
        //    for a list past nbcap).  Every core-core edge is then covered: one with an end outside the
        //    giant is processed by that end (the lists are symmetric), one inside joins nothing new.
        //    The partition is the core-point connectivity whatever the union order (union-find, min
        //    roots); the pair pass measured 58 of its 131 us per slot uniting every pair speculatively.
        if (t == 0) s_ndef = 0;
        for (int q = t; q < n; q += T) {
            if (nb_cnt(sflag[q]) < pr.minpts) continue;
            // slots 0..7; slot 1 is the first sampled link: the first neighbour of a pair list (slot 0 is
            // self there), the second entry in walk order of an own-walk list (which may be self: skipped
            // below).  A core point has cnt >= minpts entries, so slot 1 is a stored entry only for
            // minpts >= 2 (DBSCAN's 4 here): with minpts 1 a one-entry own-walk list would give its zero
            // padding, position 0, and a pair list a stale slot
            const uint4 w0 = reinterpret_cast<const uint4 *>(nbw)[q];
            const int cand[3] = {static_cast<int>(((w0.x >> 16) & 0xFFFFu) & kNbPos<N>), sX[q], slab[q]};
#pragma unroll
            for (int r = 0; r < 3; r++) {
                const int q2 = cand[r];
                if (q2 != q && q2 < n && nb_cnt(sflag[q2]) >= pr.minpts) uf_unite_s(spar, q, q2);
            }
        }
        bar();
        if (t < 64) {  // wave 0: the most frequent root among 64 core points spread over the slot
            const int q = static_cast<int>((static_cast<long long>(t) * n) >> 6);
            const int r = (q < n && nb_cnt(sflag[q]) >= pr.minpts) ? uf_find_s(spar, q) : -1;
            int best = -1, bestc = 0;
            unsigned long long act = __ballot(r >= 0);
            while (act) {
                const int L = __ffsll(static_cast<long long>(act)) - 1;
                const int rr = __shfl(r, L, 64);
                const unsigned long long m = __ballot(r == rr);
                const int c = __popcll(m);
                if (c > bestc) {
                    bestc = c;
                    best = rr;
                }
                act &= ~m;
            }
            if (t == 0) s_slot = best;  // (s_slot is free until the next ticket)
        }
        bar();
        {
            const int giant = s_slot;
            for (int q = t; q < n; q += T) {
                const int cnt = nb_cnt(sflag[q]);
                if (cnt < pr.minpts) continue;
                int ra = uf_find_s(spar, q);
                if (giant >= 0 && ra == uf_find_s(spar, giant)) continue;
                if (cnt > pr.nbcap) {
                    sX[atomicAdd(&s_ndef, 1)] = q;
                    continue;
                }
                nb_load<N>(nbw, q, cnt, w);
                // the next entry's count and union-find parent are loaded before this one's find (a parent
                // read early is still a node of q2's component, so it is a valid place to start the find)
                nb_walk(w, cnt,
                        [&](unsigned e) {
                            const int q2 = static_cast<int>(e & kNbPos<N>);
                            return make_int2(sflag[q2], ld_wg(spar + q2));
                        },
                        [&](int, unsigned e, int2 fp) {
                            const int q2 = static_cast<int>(e & kNbPos<N>);
                            if (q2 != q && nb_cnt(fp.x) >= pr.minpts && fp.y != ra) {  // parent == root: joined already
                                const int rb = uf_find_s(spar, fp.y);
                                if (rb != ra) {
                                    uf_unite_s(spar, ra, rb);
                                    ra = uf_find_s(spar, ra);
                                }
                            }
                        });
            }
        }
        bar();
        for (int f = t; f < s_ndef; f += T) {
            const int q = sX[f];
            int x, y, z;
            unpack3(keyof(q), x, y, z);
            const double ax = spt[q].x, ay = spt[q].y, az = spt[q].z;
            int ra = uf_find_s(spar, q);
            lds_cells27(g, x, y, z, 0ull, ax, ay, az, [&](int q2, double d2) {
                if (d2 < pr.eps2 && q2 != q && nb_cnt(sflag[q2]) >= pr.minpts) {
                    const int rb = uf_find_s(spar, q2);
                    if (rb != ra) {
                        uf_unite_s(spar, ra, rb);
                        ra = uf_find_s(spar, ra);
                    }
                }
            });
        }
        bar();
        BP_STAMP(22);
        // 7. roots; every component keyed by its smallest original index; clusters ranked by it
        {
            int rq[(N + T - 1) / T];
#pragma unroll
            for (int k = 0; k < (N + T - 1) / T; k++) {
                const int q = t + k * T;
                rq[k] = (q < n && nb_cnt(sflag[q]) >= pr.minpts) ? uf_find_s(spar, q) : -1;
            }
            bar();
            for (int q = t; q < n; q += T) sB[q] = INT_MAX;
            for (int x = t; x <= n; x += T) ccnt[x] = 0;
#pragma unroll
            for (int k = 0; k < (N + T - 1) / T; k++) {
                const int q = t + k * T;
                if (q < n) spar[q] = rq[k];
            }
            bar();
            for (int q = t; q < n; q += T)
                if (spar[q] >= 0) atomicMin(&sB[spar[q]], static_cast<int>(sorig[q]));
            bar();
            int carry = 0;
            for (int i0 = 0; i0 < n; i0 += T) {
                const int i = i0 + t;
                int isr = 0, r = -1;
                if (i < n) {
                    r = spar[spos[i]];
                    isr = (r >= 0 && sB[r] == i) ? 1 : 0;
                }
                int tot;
                const int ex = block_excl_scan<T>(isr, ws, tot);
                if (isr) sX[r] = carry + ex;  // rank stored at the root position
                carry += tot;
            }
        }
        bar();
        BP_STAMP(23);
        if constexpr (MC_DBG_CHECK) bp_dbg_union<N>(g, spar, n, pr, s);
        // 8. labels and class counts (a border point joins the adjacent cluster of smallest key)
        for (int q = t; q < n; q += T) {
            int l;
            if (spar[q] >= 0) {
                l = sX[spar[q]];
            } else {
                const int cnt = nb_cnt(sflag[q]);
                int best = INT_MAX, broot = -1;
                auto near = [&](int q2) {
                    const int r2 = spar[q2];
                    if (r2 >= 0 && sB[r2] < best) {
                        best = sB[r2];
                        broot = r2;
                    }
                };
                if (cnt <= pr.nbcap) {
                    nb_load<N>(nbw, q, cnt, w);
                    nb_walk(w, cnt, [](unsigned e) { return e; },
                            [&](int, unsigned e, unsigned) { near(static_cast<int>(e & kNbPos<N>)); });
                } else {
                    int x, y, z;
                    unpack3(keyof(q), x, y, z);
                    const double ax = spt[q].x, ay = spt[q].y, az = spt[q].z;
                    lds_cells27(g, x, y, z, 0ull, ax, ay, az, [&](int q2, double d2) {
                        if (d2 < pr.eps2) near(q2);
                    });
                }
                l = broot >= 0 ? sX[broot] : -1;
            }
            slab[q] = l;
            atomicAdd(&ccnt[l + 1], 1);
        }
        bar();
        BP_STAMP(24);
        // 9. class filter; S in original index order; kept rank per sorted position
        const double lim = pr.frac * static_cast<double>(n);
        for (int q = t; q < n; q += T)
            if (!(static_cast<double>(ccnt[slab[q] + 1]) < lim)) {
                sflag[q] |= 1 << 30;
                spt[q].w = __longlong_as_double(static_cast<long long>(keyof(q) | kKeptBit));
            }
        bar();
        int m = 0;
        for (int i0 = 0; i0 < n; i0 += T) {
            const int i = i0 + t;
            const int keep = (i < n && (sflag[spos[i]] & (1 << 30))) ? 1 : 0;
            int tot;
            const int ex = block_excl_scan<T>(keep, ws, tot);
            if (keep) {
                sX[m + ex] = i;
                gsx[base + m + ex] = i;   // rank -> original index, for k_bp_denoise_tail
                spar[spos[i]] = m + ex;
            }
            m += tot;
        }
        bar();
        BP_STAMP(25);
        const bool all_kept = m == n;
        // 10. k nearest kept points, the list pass: a point whose eps list holds >= k kept points
        //     takes the k nearest among them (every other kept point is >= eps away).  The others (a
        //     list longer than nbcap, or fewer than k kept entries) are deferred to the batch's
        //     ring-search kernel (k_bp_knn_ring: after every class, a lane per point over the whole
        //     chip, instead of the few lanes of one wave while the rest of this workgroup waits at a
        //     barrier), with the slot's cell grid written out for it; a slot of m < k kept points
        //     takes its whole-cloud means here.  The means go to the slot's range of gavg; the cloud
        //     statistics and the survivors follow in k_bp_denoise_tail (a wave per slot).
        const int kk = min(pr.knn, m);
        int *const sring = sB + N;  // deferred positions (sB is free after the filter)
        if (t == 0) {
            sfb[kFbCount] = 0;
            s_ndef = 0;
        }
        bar();
        double *const mavg = gavg + base;
        for (int q = t; q < n; q += T) {
            const int fl = sflag[q];
            if (!(fl & (1 << 30))) continue;
            const int r = spar[q];
            const int cnt = nb_cnt(fl);
            if (kk != kBpKnnMax) {
                sfb[atomicAdd(&sfb[kFbCount], 1)] = r;
                continue;
            }
            if (cnt > pr.nbcap) {
                sring[atomicAdd(&s_ndef, 1)] = q;
                continue;
            }
            // the k smallest squared distances, ascending, in the first k elements (the 16-class formats:
            // the sorting network's whole array, no list beside it)
            double best[kNbFine<N> ? mc::kKnnNet : kBpKnnMax];
            const double4 a = spt[q];
            auto d2of = [&](const double4 &p) {
                const double ex = a.x - p.x, ey = a.y - p.y, ez = a.z - p.z;
                return ((ex * ex) + (ey * ey)) + (ez * ez);
            };
            // selection pass: pm = the kept candidates the k nearest are among (bit k = slot k), from the
            // entries' distance classes: if >= k kept entries have a class <= c*, every other kept
            // candidate is at least as far as all of them, so only those are sorted.  Kept flags (bit 30
            // of sflag, the next one loaded ahead) are read only when the class filter dropped points.
            unsigned long long pm = 0, mall = 0;
            if constexpr (!kNbFine<N>) {
#pragma unroll
                for (int k = 0; k < kBpKnnMax; k++) best[k] = DBL_MAX;
            }
            nb_load<N>(nbw, q, cnt, w);
            auto kept_of = [&](unsigned e) { return all_kept ? 1 << 30 : sflag[e & kNbPos<N>]; };
            if constexpr (kNbFine<N>) {
                // 16 classes: a histogram of the kept entries' classes gives the smallest c* that k of
                // them reach (mc_bp_knnsel.hpp); a second walk over the register words collects them
                mc::KnnHist hist;
                nb_walk(w, cnt, kept_of, [&](int k, unsigned e, int f) {
                    const unsigned on = (static_cast<unsigned>(f) >> 30) & 1u;
                    mall |= static_cast<unsigned long long>(on) << k;
                    hist.add(e >> kNbShift<N>, on);
                });
                const int cstar = mc::knn_threshold(hist, kk);  // -1: fewer than k kept entries
                nb_walk(w, cnt, [](unsigned e) { return e; }, [&](int k, unsigned e, unsigned) {
                    pm |= static_cast<int>(e >> kNbShift<N>) <= cstar ? 1ull << k : 0ull;
                });
                pm &= mall;
            } else {
                // three radii (m1 / m2 / m3): the smallest of the nested sets that holds k
                unsigned long long m1 = 0, m2 = 0, m3 = 0;
                nb_walk(w, cnt, kept_of, [&](int k, unsigned e, int f) {
                    const unsigned long long bit = (f & (1 << 30)) ? 1ull << k : 0ull;
                    const unsigned c = e >> kNbShift<N>;
                    mall |= bit;
                    m1 |= c == 0u ? bit : 0ull;
                    m2 |= c <= 1u ? bit : 0ull;
                    m3 |= c <= 2u ? bit : 0ull;
                });
                pm = __popcll(m1) >= kk ? m1 : __popcll(m2) >= kk ? m2 : __popcll(m3) >= kk ? m3 : mall;
            }
            const int found = __popcll(mall);
#ifdef MC_BP_STAMPS
            // (every point of the pass, the deferred ones included, in both entry formats)
            atomicAdd(&g_bp_stamps[29], static_cast<unsigned long long>(found));
            atomicAdd(&g_bp_stamps[13], 1ull);
#endif
#ifdef MC_BP_STAMPS_SEL
            bp_stamp_selected(found >= kk ? __popcll(pm) : 0);
#endif
            if constexpr (kNbFine<N>) {
                // fewer than k kept entries: the ring queue's.  The 16-class format leaves here, before the
                // array is written: an array that reaches the sum below undefined on one path and sorted on
                // the other cost the pass spills inside this loop.  (The 2-bit format defers after its
                // insert loop, below, as it always did.)
                if (found < kk) {
                    sring[atomicAdd(&s_ndef, 1)] = q;
                    continue;
                }
            }
            if (kNbFine<N> || found >= kk) {  // (16-class format: always, found >= kk from here on)
                // slot k of q: byte (((k / 8) * N + q) * 8 + k % 8) * 2 of the region (32-bit offsets
                // from the workgroup's base, as nb_put)
                const char *lstb = reinterpret_cast<const char *>(nbw);
                const unsigned qb = static_cast<unsigned>(q) * 16u;
                // the selected entries' positions are reloaded from the list (a lane-varying slot index
                // cannot read the register copy), kBpKnnBatch at a time, the next batch's loads in flight
                // while this batch's points are inserted: the lists live past the L2 (one region per
                // workgroup), and one load in flight per lane left the pass waiting on every entry
                auto fetch = [&](int (&e)[kBpKnnBatch]) {
#pragma unroll
                    for (int u = 0; u < kBpKnnBatch; u++) {
                        const int b = pm ? __ffsll(static_cast<long long>(pm)) - 1 : -1;
                        pm &= pm - 1;
                        const unsigned ob = (static_cast<unsigned>(b) >> 3) * (16u * static_cast<unsigned>(N)) + qb +
                                            ((static_cast<unsigned>(b) & 7u) << 1);
                        e[u] = b >= 0 ? static_cast<int>(*reinterpret_cast<const unsigned short *>(lstb + ob)) : -1;
                    }
                };
                if constexpr (kNbFine<N>) {
                    // one round: the first kKnnNet selected entries, every load issued before the first
                    // use (a selected set is 20 .. ~24 entries: no trip loop whose length is the wave's
                    // largest set, no chain of dependent reloads).  An absent entry reads slot 0 (a valid
                    // address: every list holds its point) and is marked -1: no branch around a load.
                    int en[mc::kKnnNet];
#pragma unroll
                    for (int u = 0; u < mc::kKnnNet; u++) {
                        const unsigned b = pm ? static_cast<unsigned>(__ffsll(static_cast<long long>(pm)) - 1) : 0u;
                        const unsigned ob = (b >> 3) * (16u * static_cast<unsigned>(N)) + qb + ((b & 7u) << 1);
                        const int e = static_cast<int>(*reinterpret_cast<const unsigned short *>(lstb + ob));
                        en[u] = pm ? e : -1;
                        pm &= pm - 1;
                    }
                    // their squared distances straight into the sorting network's array, DBL_MAX for the
                    // absent ones; the network leaves the array's first k elements the k smallest, ascending
#pragma unroll
                    for (int u = 0; u < mc::kKnnNet; u++) {
                        const double v = d2of(spt[en[u] >= 0 ? en[u] & kNbPos<N> : q]);
                        best[u] = en[u] >= 0 ? v : DBL_MAX;
                    }
                    mc::knn_net_sort(best, [](double &lo, double &hi) {
                        const double x = lo, y = hi;
                        lo = ins_min(x, y);
                        hi = ins_max(x, y);
                    });
                    // leftovers (a set larger than the network, rare): the batched insert loop on the
                    // sorted first k, entered only if some lane of the wave has any
                    if (__ballot(pm != 0ull)) {
                        int el[kBpKnnBatch];
                        fetch(el);
                        while (el[0] >= 0) {
                            double d2[kBpKnnBatch];
#pragma unroll
                            for (int u = 0; u < kBpKnnBatch; u++) {
                                const double4 p = spt[el[u] >= 0 ? el[u] & kNbPos<N> : q];
                                d2[u] = el[u] >= 0 ? d2of(p) : DBL_MAX;
                            }
                            fetch(el);
#pragma unroll
                            for (int u = 0; u < kBpKnnBatch; u++)
                                mc::knn_insert<kBpKnnMax>(
                                    best, d2[u], [](double x, double y) { return ins_min(x, y); },
                                    [](double x, double y) { return ins_max(x, y); });
                        }
                    }
                } else {
                    int en[kBpKnnBatch];
                    fetch(en);
                    while (en[0] >= 0) {
                        double d2[kBpKnnBatch];
#pragma unroll
                        for (int u = 0; u < kBpKnnBatch; u++) {
                            const double4 p = spt[en[u] >= 0 ? en[u] & kNbPos<N> : q];
                            d2[u] = en[u] >= 0 ? d2of(p) : DBL_MAX;
                        }
                        fetch(en);
#pragma unroll
                        for (int u = 0; u < kBpKnnBatch; u++) sorted_insert(best, d2[u]);
                    }
                }
            }
            if constexpr (!kNbFine<N>) {  // (the 16-class format deferred these points above)
                if (found < kk) {
                    sring[atomicAdd(&s_ndef, 1)] = q;
                    continue;
                }
            }
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < kBpKnnMax; k++) sum = sum + sqrt(best[k]);
            mavg[r] = sum / static_cast<double>(kk);
            bp_dbg_path(static_cast<size_t>(base) + r, 1u | (static_cast<unsigned>(N) << 4) | (static_cast<unsigned>(cnt) << 20));
        }
        bar();
        BP_STAMP(34);  // k-NN: the list pass
#ifdef MC_BP_STAMPS
        if (t == 0) atomicAdd(&g_bp_stamps[30], static_cast<unsigned long long>(s_ndef));
#endif
        // m < k kept points: every kept point's mean over the whole cloud, a wave per point
        const int nfb = sfb[kFbCount];
        for (int f = wv; f < nfb; f += NW) {
            const int r = sfb[f];
            const double4 a = spt[spos[sX[r]]];
            const double mean = wave_knn_mean(m, kk, [&](int j) {
                const double4 p = spt[spos[sX[j]]];
                const double ex = a.x - p.x, ey = a.y - p.y, ez = a.z - p.z;
                return ((ex * ex) + (ey * ey)) + (ez * ez);
            });
            if (lane == 0) {
                mavg[r] = mean;
                bp_dbg_path(static_cast<size_t>(base) + r, 2u | (static_cast<unsigned>(N) << 4));
            }
        }
        // the deferred points: the slot's grid (cell-sorted records with kept bits, bucket starts,
        // origin and extent) to its own ranges, its points to the batch's ring-search queue (slot,
        // position | rank << 14; at most one entry per voxel of the batch, so a pixel-sized array holds it)
        const int nd = s_ndef;
        if (nd > 0) {
            double4 *gr = grec + base;
            for (int i = t; i < n; i += T) gr[i] = spt[i];
            int *gb = gbs + 2 * static_cast<size_t>(base) + s;
            for (int b = t; b <= NBK * n; b += T) gb[b] = sA[b];
            // the queue holds at most one entry per voxel of the batch, so a pixel-sized array cannot
            // fill; a region past its end is an internal error, reported (BS_DNERR) instead of written
            if (t == 0) s_slot = atomicAdd(dq_cnt, nd);  // (s_slot is read again only after the next ticket)
            bar();
            const int e0 = s_slot;
            if (e0 > dq_cap - nd) {
                if (t == 0) atomicOr(err, 2);
            } else
            for (int f = t; f < nd; f += T) {
                const int q = sring[f];
                dq[e0 + f] = s;
                gitem[e0 + f] = q | (spar[q] << 14);
            }
            if (MC_DBG_CHECK && t == 0) {  // the origin handed to the ring kernel against the records' keys
                double fm[3] = {DBL_MAX, DBL_MAX, DBL_MAX};
                for (int i = 0; i < n; i++)
                    for (int c = 0; c < 3; c++) fm[c] = fmin(fm[c], P[3 * i + c]);
                for (int i = 0; i < n; i++) {
                    int kx, ky, kz;
                    unpack3(static_cast<unsigned long long>(__double_as_longlong(spt[i].w)) & ~kKeptBit, kx, ky, kz);
                    const int cz = static_cast<int>(floor((spt[i].z - mn[2]) / pr.ce));
                    const int cy = static_cast<int>(floor((spt[i].y - mn[1]) / pr.ce));
                    if ((cz != kz || cy != ky) && bp_dbg_fail(5)) {
                        printf("[bp dbg origin] N=%d slot=%d n=%d rec %d key (%d,%d,%d) from mn (%d,%d); mn (%.17g,%.17g,%.17g) "
                               "fresh min (%.17g,%.17g,%.17g)\n", N, s, n, i, kx, ky, kz, cy, cz, mn[0], mn[1], mn[2], fm[0], fm[1],
                               fm[2]);
                        break;
                    }
                }
            }
        }
#ifdef MC_BP_STAMPS
        if (t == 0 && s < (1 << 16)) g_bp_slot_time[s] = static_cast<unsigned>(__builtin_amdgcn_s_memrealtime() - slot_t0);
#endif
        if (t == 0) slot_m[s] = m;
        bar();
    }
}

}  // namespace mc
