// mc_bp_knnsel.hpp — S1 denoise: the k-NN list pass's candidate selection in the LDS classes of up to
// 4096 points (k_bp_denoise_lds, mc_bp_denoise_lds.inl, step 10).  Plain C++17 without a HIP include, usable
// from host and device; scripts/bp_knnsel_check.cpp checks it on the CPU (tests/test_bp_knnsel_cpu.py).
//  * knn_class(d2, s) is the distance class of an eps-list entry, 0 .. 15, stored in the entry's top four
//    bits: min(15, (unsigned)(d2 * s)) with s = 16 / eps2 (knn_scale, computed once on the host).  It is a
//    function of d2 alone and monotone non-decreasing in it: a rounded multiply by a positive constant, a
//    truncation and a min are each monotone.  That is the whole correctness argument of the selection: if
//    at least kk kept entries of a list have class <= c*, an entry of a higher class has a d2 at least as
//    large as each of theirs, so the kk smallest distances are all found among the entries of class <= c*
//    (as values: equal distances are interchangeable).
//  * KnnHist counts a point's kept entries per class: sixteen byte counters (a list has <= 64 entries) in
//    four 32-bit words with static names, no indexed register array.  knn_threshold(hist, kk) is the
//    smallest c* whose cumulative count reaches kk, or -1 if the total is below kk.
//  * knn_net_sort sorts kKnnNet values with a fixed comparator list: Batcher's odd-even merge sort of 32
//    lines (in its merge-exchange form), generated at compile time, without the lines from kKnnNet up and
//    their comparators (those lines would carry +inf, which no comparator moves down).  The pass reads
//    outputs 0 .. kKnnOut - 1 only; the comparators that feed nothing else are left to the compiler's
//    dead-code elimination.
//  * knn_insert is the sorted insert of the leftover entries (a point with more than kKnnNet selected
//    entries) into the first K elements of the sorted array.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

#if defined(__HIPCC__)
#define MC_KS_HD __host__ __device__ __forceinline__
#define MC_KS_UNROLL _Pragma("unroll")
#else
#define MC_KS_HD inline
#define MC_KS_UNROLL
#endif

namespace mc {

constexpr int kKnnClasses = 16;  // distance classes of an entry (four bits)
constexpr int kKnnNet = 24;      // inputs of the sorting network (selected entries fetched in one round)
constexpr int kKnnOut = 20;      // outputs read: kBpKnnMax

// the class scale of a squared radius
inline double knn_scale(double eps2) { return static_cast<double>(kKnnClasses) / eps2; }

// 0 <= d2 (no NaN), d2 * s far below 2^32
MC_KS_HD unsigned knn_class(double d2, double s)
{
    const unsigned c = static_cast<unsigned>(d2 * s);
    return c < static_cast<unsigned>(kKnnClasses - 1) ? c : static_cast<unsigned>(kKnnClasses - 1);
}

struct KnnHist {
    uint32_t h0 = 0, h1 = 0, h2 = 0, h3 = 0;  // byte c % 4 of word c / 4: entries of class c

    // on = 1 counts the entry, 0 leaves the histogram as it is
    MC_KS_HD void add(unsigned c, uint32_t on)
    {
        const uint32_t inc = on << ((c & 3u) * 8u);
        const uint32_t g = c >> 2;
        h0 += g == 0u ? inc : 0u;
        h1 += g == 1u ? inc : 0u;
        h2 += g == 2u ? inc : 0u;
        h3 += g == 3u ? inc : 0u;
    }
    MC_KS_HD unsigned count(unsigned c) const
    {
        const uint32_t g = c >> 2;
        const uint32_t w = g == 0u ? h0 : g == 1u ? h1 : g == 2u ? h2 : h3;
        return (w >> ((c & 3u) * 8u)) & 0xFFu;
    }
};

// the smallest class whose cumulative count is >= kk (1 <= kk <= 64; the counts sum to <= 64), or -1.
// A multiply by 0x01010101 leaves in byte j the sum of bytes 0 .. j (sums <= 64: no carry between bytes);
// adding 128 - kk to every byte sets its top bit where the cumulative count has reached kk (<= 64 + 127).
MC_KS_HD int knn_threshold(const KnnHist &h, int kk)
{
    constexpr uint32_t ones = 0x01010101u;
    const uint32_t p0 = h.h0 * ones;
    const uint32_t p1 = h.h1 * ones + (p0 >> 24) * ones;
    const uint32_t p2 = h.h2 * ones + (p1 >> 24) * ones;
    const uint32_t p3 = h.h3 * ones + (p2 >> 24) * ones;
    const uint32_t bias = static_cast<uint32_t>(128 - kk) * ones;
    const uint32_t m0 = (p0 + bias) & 0x80808080u, m1 = (p1 + bias) & 0x80808080u, m2 = (p2 + bias) & 0x80808080u,
                   m3 = (p3 + bias) & 0x80808080u;
    const uint32_t m = m0 ? m0 : m1 ? m1 : m2 ? m2 : m3;
    if (!m) return -1;
    const int word = m0 ? 0 : m1 ? 1 : m2 ? 2 : 3;
    const int byte = (m & 0x80u) ? 0 : (m & 0x8000u) ? 1 : (m & 0x800000u) ? 2 : 3;
    return 4 * word + byte;
}

// ---- the sorting network ----
struct KnnNetList {
    int n = 0;
    unsigned char a[192] = {}, b[192] = {};  // comparator i orders lines a[i] < b[i]
};

// Batcher's odd-even merge sort of `lines` (a power of two) lines as merge exchange (Knuth 5.2.2, Algorithm
// M); the comparators that touch a line >= keep are left out
constexpr KnnNetList knn_make_net(int lines, int keep)
{
    KnnNetList net;
    for (int p = 1; p < lines; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= lines - 1 - k; j += 2 * k)
                for (int i = 0; i <= (k - 1 < lines - j - k - 1 ? k - 1 : lines - j - k - 1); i++)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p) && i + j + k < keep) {
                        net.a[net.n] = static_cast<unsigned char>(i + j);
                        net.b[net.n] = static_cast<unsigned char>(i + j + k);
                        net.n++;
                    }
    return net;
}
constexpr KnnNetList kKnnNetList = knn_make_net(32, kKnnNet);

template <size_t I>
struct KnnCmp {
    static constexpr int a = kKnnNetList.a[I], b = kKnnNetList.b[I];
};
template <typename V, typename Cx, size_t... I>
MC_KS_HD void knn_net_run(V (&d)[kKnnNet], Cx &&cx, std::index_sequence<I...>)
{
    (cx(d[KnnCmp<I>::a], d[KnnCmp<I>::b]), ...);  // static line numbers: no indexed register array
}
// cx(lo, hi) leaves the smaller of its two values in lo and the larger in hi
template <typename V, typename Cx>
MC_KS_HD void knn_net_sort(V (&d)[kKnnNet], Cx &&cx)
{
    knn_net_run(d, cx, std::make_index_sequence<static_cast<size_t>(kKnnNetList.n)>{});
}

// sorted insert of v into the ascending a[0 .. K) (drops the largest): new a[q] = min(a[q], max(a[q-1], v))
template <int K, int M, typename V, typename Mn, typename Mx>
MC_KS_HD void knn_insert(V (&a)[M], V v, Mn &&mn, Mx &&mx)
{
    static_assert(K <= M, "the sorted prefix lies inside the array");
    if (!(v < a[K - 1])) return;
    MC_KS_UNROLL
    for (int q = K - 1; q > 0; q--) a[q] = mn(a[q], mx(a[q - 1], v));
    a[0] = mn(a[0], v);
}

}  // namespace mc
